// Geometry, blend and DDIM-update kernels of the Mixer step (gfx950).  HBM-bound elementwise work over
// [n, T, 2 persons, 262] motion tensors; one thread per (sample, person, frame, joint) so that the 21 rotation
// round trips (6D -> matrix -> quaternion -> axis-angle -> quaternion -> matrix -> 6D) spread over lanes.
//
// Reference restated here (value-for-value, branch-free versions of the reference's masked-index code):
//   src/utils/alignment.py:11-67 (ih_to_smpl / smpl_to_ih), :69-158 (align_trajectories / align_motions), :161-222 (center_motion)
//   src/utils/rotation_conversions.py:38-120, 449-571;  src/utils/quaternion.py:54-73 (qrot), 386-396 (qbetween)
//   src/utils/utils.py:44-82 (normalisers);  src/models/mixermdm.py:691-801;  src/models/utils/cfg_sampler.py:49-55
//   src/models/utils/gaussian_diffusion.py:2031-2062 (process_xstart), 1936-1965 (two-chain DDIM, eta = 0), 558-562
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.h"

namespace {

constexpr int NF = MMDM_NF;          // 262
constexpr int NF2 = 2 * MMDM_NF;     // 524
constexpr int NJ = MMDM_NJ;          // 22
constexpr int ROT0 = 132;            // first rot6d channel
constexpr int FEET0 = 258;
constexpr int R_HIP = 2, L_HIP = 1;  // FACE_JOINT_INDX[:2]  src/utils/paramUtil.py:89

struct V3 { float x, y, z; };
struct Q4 { float w, x, y, z; };

__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// quaternion.py:54-73
__device__ __forceinline__ V3 qrot(Q4 q, V3 v) {
    const V3 qv{q.x, q.y, q.z};
    const V3 uv = cross3(qv, v);
    const V3 uuv = cross3(qv, uv);
    return V3{v.x + 2.f * (q.w * uv.x + uuv.x), v.y + 2.f * (q.w * uv.y + uuv.y), v.z + 2.f * (q.w * uv.z + uuv.z)};
}

// quaternion.py:386-396 + qnormalize :28-30
__device__ __forceinline__ Q4 qbetween(V3 a, V3 b) {
    const V3 v = cross3(a, b);
    const float w = sqrtf((a.x * a.x + a.y * a.y + a.z * a.z) * (b.x * b.x + b.y * b.y + b.z * b.z)) + (a.x * b.x + a.y * b.y + a.z * b.z) + 1e-8f;
    const float n = sqrtf(w * w + v.x * v.x + v.y * v.y + v.z * v.z);
    return Q4{w / n, v.x / n, v.y / n, v.z / n};
}

__device__ __forceinline__ float sqrt_pos(float x) { return x > 0.f ? sqrtf(x) : 0.f; }                 // rotation_conversions.py:85-95
__device__ __forceinline__ float copysign_ref(float a, float b) { return ((a < 0.f) != (b < 0.f)) ? -a : a; }  // :68-82
__device__ __forceinline__ float half_sinc(float half, float ang) {                                      // :466-475 / :497-507
    return (fabsf(ang) < 1e-6f) ? (0.5f - (ang * ang) / 48.f) : (sinf(half) / ang);
}

// rot6d (interleaved) -> rot6d after the ih_to_smpl -> smpl_to_ih round trip (the two "* -1" cancel exactly).
__device__ __forceinline__ void rot6d_roundtrip(const float d[6], float out[6]) {
    // rotation_6d_to_matrix :511-534 (a1 = d[0,2,4], a2 = d[1,3,5]; F.normalize eps 1e-12)
    float a1x = d[0], a1y = d[2], a1z = d[4], a2x = d[1], a2y = d[3], a2z = d[5];
    float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);
    const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
    const float dt = b1x * a2x + b1y * a2y + b1z * a2z;
    float b2x = a2x - dt * b1x, b2y = a2y - dt * b1y, b2z = a2z - dt * b1z;
    const float n2 = fmaxf(sqrtf(b2x * b2x + b2y * b2y + b2z * b2z), 1e-12f);
    b2x /= n2; b2y /= n2; b2z /= n2;
    const float b3x = b1y * b2z - b1z * b2y, b3y = b1z * b2x - b1x * b2z, b3z = b1x * b2y - b1y * b2x;
    // rows: m0 = b1, m1 = b2, m2 = b3.   matrix_to_quaternion :98-120
    const float m00 = b1x, m01 = b1y, m02 = b1z, m10 = b2x, m11 = b2y, m12 = b2z, m20 = b3x, m21 = b3y, m22 = b3z;
    const float qw = 0.5f * sqrt_pos(1.f + m00 + m11 + m22);
    const float qx = copysign_ref(0.5f * sqrt_pos(1.f + m00 - m11 - m22), m21 - m12);
    const float qy = copysign_ref(0.5f * sqrt_pos(1.f - m00 + m11 - m22), m02 - m20);
    const float qz = copysign_ref(0.5f * sqrt_pos(1.f - m00 - m11 + m22), m10 - m01);
    // quaternion_to_axis_angle :480-508
    const float nrm = sqrtf(qx * qx + qy * qy + qz * qz);
    const float half = atan2f(nrm, qw);
    const float ang = 2.f * half;
    const float s1 = half_sinc(half, ang);
    const float ax = qx / s1, ay = qy / s1, az = qz / s1;     // (ih_to_smpl's *-1 and smpl_to_ih's *-1 cancel)
    // axis_angle_to_quaternion :449-477
    const float ang2 = sqrtf(ax * ax + ay * ay + az * az);
    const float half2 = 0.5f * ang2;
    const float s2 = half_sinc(half2, ang2);
    const float r = cosf(half2), i = ax * s2, j = ay * s2, k = az * s2;
    // quaternion_to_matrix :38-65 (first two rows), matrix_to_rotation_6d :540-571 (interleave)
    const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
    out[0] = 1.f - two_s * (j * j + k * k);   // m00
    out[2] = two_s * (i * j - k * r);         // m01
    out[4] = two_s * (i * k + j * r);         // m02
    out[1] = two_s * (i * j + k * r);         // m10
    out[3] = 1.f - two_s * (i * i + k * k);   // m11
    out[5] = two_s * (j * k - i * r);         // m12
}

// ---------------------------------------------------------------------------------------------------------
// Mixer pre-processing: denormalise both denoiser outputs, align the individual prediction to the interaction one.
// grid: n * 2 persons * T blocks of 32 threads?  -> flat: one thread per (b, p, t, j), j in [0, 22).
// ---------------------------------------------------------------------------------------------------------
// RAG: ragged batch (kernels.h mmdm_rag) -- `n` counts GROUPS of rg.rows frame rows (cond | uncond halves), a thread is (frame row, person, joint),
// frame 0 / the last frame of its item come from the row maps; padding rows leave at once.  The arithmetic is the uniform kernel's.
template <bool RAG>
__global__ __launch_bounds__(256) void mixer_pre_kernel(const float* __restrict__ o1, const float* __restrict__ o2, const float* __restrict__ stats,
                                                         float* __restrict__ out1, float* __restrict__ out2, int n, int T, int align, mmdm_rag rg,
                                                         const int* __restrict__ last_frame, int last_rows) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    int j, t, p;
    size_t seq;
    int tl;                                   // end frame of the alignment's displacement
    if constexpr (RAG) {
        if (idx >= n * rg.rows * 2 * NJ) return;
        j = idx % NJ;
        p = (idx / NJ) % 2;
        const int r = idx / (NJ * 2), rl = r % rg.rows, item = rg.row_item[rl];
        if (item < 0) return;
        t = rg.row_pos[rl];
        T = rg.item_len[item];
        seq = (size_t)(r - t) * NF2 + (size_t)p * NF;
        tl = T - 1;
    } else {
        const int total = n * 2 * T * NJ;
        if (idx >= total) return;
        j = idx % NJ;
        t = (idx / NJ) % T;
        p = (idx / (NJ * T)) % 2;
        const int b = idx / (NJ * T * 2);
        seq = (size_t)b * T * NF2 + (size_t)p * NF;      // start of (b, frame 0, person p)
        // mask given: frame lengths - 1 with lengths = mask.sum(dim=1) (alignment.py:89-91) -- the COUNT of valid frames, not the last valid one
        tl = last_frame ? min(max(last_frame[b % last_rows], 0), T - 1) : T - 1;
    }
    const float* mh = stats, *sh = stats + NF, *mi = stats + 2 * NF, *si = stats + 3 * NF;
    const size_t off = seq + (size_t)t * NF2;
    const float* a = o1 + off;   // individual denoiser, HML3D normalisation
    const float* c = o2 + off;   // interaction denoiser, InterHuman normalisation
    float* y1 = out1 + off;
    float* y2 = out2 + off;

    // interaction stream: pos / vel pass through (denormalised); rot6d re-orthonormalised when align
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        y2[3 * j + k] = c[3 * j + k] * si[3 * j + k] + mi[3 * j + k];
        y2[66 + 3 * j + k] = c[66 + 3 * j + k] * si[66 + 3 * j + k] + mi[66 + 3 * j + k];
    }
    if (j < 21) {
        float d[6], r[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = c[ROT0 + 6 * j + k] * si[ROT0 + 6 * j + k] + mi[ROT0 + 6 * j + k];
        if (align) rot6d_roundtrip(d, r);
#pragma unroll
        for (int k = 0; k < 6; ++k) y2[ROT0 + 6 * j + k] = align ? r[k] : d[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = a[ROT0 + 6 * j + k] * sh[ROT0 + 6 * j + k] + mh[ROT0 + 6 * j + k];
        if (align) rot6d_roundtrip(d, r);
#pragma unroll
        for (int k = 0; k < 6; ++k) y1[ROT0 + 6 * j + k] = align ? r[k] : d[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            y2[FEET0 + k] = c[FEET0 + k] * si[FEET0 + k] + mi[FEET0 + k];
            // after align_motions (201-d) smpl_to_ih appends the zero hand padding as "feet"
            y1[FEET0 + k] = align ? 0.f : (a[FEET0 + k] * sh[FEET0 + k] + mh[FEET0 + k]);
        }
    }

    V3 pos{a[3 * j] * sh[3 * j] + mh[3 * j], a[3 * j + 1] * sh[3 * j + 1] + mh[3 * j + 1], a[3 * j + 2] * sh[3 * j + 2] + mh[3 * j + 2]};
    V3 vel{a[66 + 3 * j] * sh[66 + 3 * j] + mh[66 + 3 * j], a[66 + 3 * j + 1] * sh[66 + 3 * j + 1] + mh[66 + 3 * j + 1],
           a[66 + 3 * j + 2] * sh[66 + 3 * j + 2] + mh[66 + 3 * j + 2]};
    if (align) {
        // align_motions(motion1 = interaction person (target), motion2 = individual person (moved))  alignment.py:112-158
        const float* a0 = o1 + seq;                               // frame 0
        const float* aL = o1 + seq + (size_t)tl * NF2;            // last frame (mask=None: alignment.py:86-88), or the mask's frame count - 1
        const float* c0 = o2 + seq;
        const float* cL = o2 + seq + (size_t)tl * NF2;
        const V3 p1_0{c0[0] * si[0] + mi[0], c0[1] * si[1] + mi[1], c0[2] * si[2] + mi[2]};
        const V3 p1_L{cL[0] * si[0] + mi[0], cL[1] * si[1] + mi[1], cL[2] * si[2] + mi[2]};
        const V3 p2_0{a0[0] * sh[0] + mh[0], a0[1] * sh[1] + mh[1], a0[2] * sh[2] + mh[2]};
        const V3 p2_L{aL[0] * sh[0] + mh[0], aL[1] * sh[1] + mh[1], aL[2] * sh[2] + mh[2]};
        const V3 dl{p1_0.x - p2_0.x, p1_0.y - p2_0.y, p1_0.z - p2_0.z};
        const V3 t2_0{p2_0.x + dl.x, p2_0.y + dl.y, p2_0.z + dl.z};     // translated root, frame 0
        const V3 t2_L{p2_L.x + dl.x, p2_L.y + dl.y, p2_L.z + dl.z};
        V3 v1{p1_L.x - p1_0.x, 0.f, p1_L.z - p1_0.z};
        V3 v2{t2_L.x - t2_0.x, 0.f, t2_L.z - t2_0.z};
        const float n1 = sqrtf(v1.x * v1.x + v1.y * v1.y + v1.z * v1.z + 1e-8f);
        const float n2 = sqrtf(v2.x * v2.x + v2.y * v2.y + v2.z * v2.z + 1e-8f);
        v1 = V3{v1.x / n1, v1.y / n1, v1.z / n1};
        v2 = V3{v2.x / n2, v2.y / n2, v2.z / n2};
        const Q4 q = qbetween(v2, v1);
        const V3 r0 = qrot(q, t2_0);                                     // rotated root, frame 0
        const V3 d2{p1_0.x - r0.x, p1_0.y - r0.y, p1_0.z - r0.z};
        const V3 pr = qrot(q, V3{pos.x + dl.x, pos.y + dl.y, pos.z + dl.z});
        pos = V3{pr.x + d2.x, pr.y + d2.y, pr.z + d2.z};
        vel = qrot(q, vel);
    }
    y1[3 * j] = pos.x; y1[3 * j + 1] = pos.y; y1[3 * j + 2] = pos.z;
    y1[66 + 3 * j] = vel.x; y1[66 + 3 * j + 1] = vel.y; y1[66 + 3 * j + 2] = vel.z;
}

// ---------------------------------------------------------------------------------------------------------
// Influence expansion + blend + CFG combine.  One thread per (b, t, channel c in [0,524)).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int influence_index(int c) {   // 262 channels -> 23 groups  mixermdm.py:767-784
    return c < 66 ? c / 3 : (c < 132 ? (c - 66) / 3 : (c < FEET0 ? (c - ROT0) / 6 : 22));
}

// History side outputs under graph replay.  The destination pointers and the stride live in a DEVICE-side descriptor (mmdm_hist_desc,
// kernels.h) that the kernels read at run time, so a captured step graph does not depend on them: the same graph serves calls with
// different (or no) history buffers, and a stale buffer can never be baked into a replayed node.
// slot = *loop_pos / every when *loop_pos % every == 0, else none.
__device__ __forceinline__ long hist_slot(const int* loop_pos, int every) {
    if (!loop_pos) return 0;
    const int lp = *loop_pos;
    return (lp % every == 0) ? (long)(lp / every) : -1;
}

// hd != nullptr: history pointers / stride come from the descriptor (the explicit pointer arguments are ignored).
// nwh: channels of an influence history row: 262 (modes 3, 4: the expanded tensor) or 1 (modes 1, 2: the reference appends the
// un-expanded [2B, T, 1] tensor, mixermdm.py:739-745, 794-796).
template <bool RAG>
__global__ __launch_bounds__(256) void blend_cfg_kernel(const float* __restrict__ out1, const float* __restrict__ out2, const float* __restrict__ w,
                                                         int Tw, int nw, int use_force, float force, float s,
                                                         float* __restrict__ model_out, float* __restrict__ hist_i1, float* __restrict__ hist_i2,
                                                         float* __restrict__ hist_mix, const mmdm_hist_desc* __restrict__ hd,
                                                         const int* __restrict__ loop_pos, int nwh, int B, int T, mmdm_rag rg) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // frames of one half of the CFG-doubled batch: B * T, or the ragged batch's group stride (padding rows included: history slots are [2 * rows, C])
    const size_t half = RAG ? (size_t)rg.rows : (size_t)B * T;
    const size_t total = half * NF2;
    if (idx >= total) return;
    int every = 1;
    if (hd) { hist_i1 = hd->i1; hist_i2 = hd->i2; hist_mix = hd->mix; every = hd->every; }
    const long slot = hist_slot(loop_pos, every);
    if (slot < 0) { hist_i1 = nullptr; hist_i2 = nullptr; hist_mix = nullptr; }
    else {
        if (hist_i1) hist_i1 += (size_t)slot * 2 * half * nwh;
        if (hist_i2) hist_i2 += (size_t)slot * 2 * half * nwh;
        if (hist_mix) hist_mix += (size_t)slot * 2 * half * NF2;
    }
    const int ch = (int)(idx % NF2);
    const size_t fr = idx / NF2;                        // frame row inside the half
    int b;
    if constexpr (RAG) { b = rg.row_item[fr]; if (b < 0) return; }
    else b = (int)(fr / T);
    const int p = ch >= NF ? 1 : 0;
    const int c = ch - p * NF;
    const int wi = nw == 1 ? 0 : influence_index(c);
    float mix[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {                       // u = 0: cond row b, u = 1: uncond row B + b
        const size_t frow = (size_t)u * half + fr;      // frame row of the doubled batch (= (b + u B) T + t in the uniform layout)
        const size_t e = frow * NF2 + ch;
        // w: [2 persons][2B sequences][Tw][nw] -- per frame (Tw = T: the Influence head's rows, person-major like the stack's) or per sequence (Tw = 1)
        float wv = Tw == 1 ? w[((size_t)p * 2 * B + (b + u * B)) * nw + wi] : w[((size_t)p * 2 * half + frow) * nw + wi];
        if (use_force) wv = 1.0f * force;
        const float v1 = out1[e], v2 = out2[e];
        mix[u] = v2 + wv * (v1 - v2);
        if (hist_mix) hist_mix[e] = mix[u];
        float* hi = p ? hist_i2 : hist_i1;
        if (hi && c < nwh) hi[frow * nwh + c] = wv;
    }
    model_out[idx] = s * mix[0] + (1.0f - s) * mix[1];
}

// ---------------------------------------------------------------------------------------------------------
// process_xstart + two-chain DDIM update.
// ---------------------------------------------------------------------------------------------------------
// floor[b, p] = min over (t, joint) of position Y   (center_motion "Put on Floor", alignment.py:182-184)
template <bool RAG>
__global__ __launch_bounds__(256) void floor_kernel(const float* __restrict__ m, float* __restrict__ floor_ws, int T, mmdm_rag rg) {
    const int bp = blockIdx.x;                   // b * 2 + p
    size_t row0 = (size_t)(bp >> 1) * T;
    if constexpr (RAG) { row0 = (size_t)rg.item_off[bp >> 1]; T = rg.item_len[bp >> 1]; }
    const float* base = m + row0 * NF2 + (size_t)(bp & 1) * NF;
    float v = INFINITY;
    for (int i = threadIdx.x; i < T * NJ; i += blockDim.x) {
        const int t = i / NJ, j = i % NJ;
        v = fminf(v, base[(size_t)t * NF2 + 3 * j + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) floor_ws[bp] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// smpl_to_ih(center_motion(ih_to_smpl(.)))  alignment.py:161-222 for the channels ONE thread owns (joint j of one frame of one person): raw / v1 hold
// pos j (3), vel j (3), then rot j (6, j < 21) or the feet (4, j == 21).  fl: the person's floor (floor_kernel / center_floor_kernel); f0: the person's
// frame 0, which supplies the root XZ and the hip-across vector.  Positions / velocities are unchanged by ih_to_smpl; the facing rotation is
// qbetween(normalize(cross(Y, across)), +Z) with the cross product along the last dimension.  One definition for the DDIM update and the evaluator's
// two centring kernels: the operation order is the update kernel's, value for value.
struct Centred { V3 pos, vel; float rot[6]; };          // rot: the rot6d of joint j < 21; zeros for j == 21 (the feet)
__device__ __forceinline__ Centred center_channels(float fl, const float* f0, int j, V3 pos, V3 vel, const float (&d)[6]) {
    const V3 root{f0[0], f0[1] - fl, f0[2]};
    const V3 rh{f0[3 * R_HIP], f0[3 * R_HIP + 1] - fl, f0[3 * R_HIP + 2]};
    const V3 lhp{f0[3 * L_HIP], f0[3 * L_HIP + 1] - fl, f0[3 * L_HIP + 2]};
    V3 ac{rh.x - lhp.x, rh.y - lhp.y, rh.z - lhp.z};
    const float an = sqrtf(ac.x * ac.x + ac.y * ac.y + ac.z * ac.z);
    ac = V3{ac.x / an, ac.y / an, ac.z / an};
    V3 fw = cross3(V3{0.f, 1.f, 0.f}, ac);
    const float fn = sqrtf(fw.x * fw.x + fw.y * fw.y + fw.z * fw.z);
    fw = V3{fw.x / fn, fw.y / fn, fw.z / fn};
    const Q4 q = qbetween(fw, V3{0.f, 0.f, 1.f});
    const V3 xz{root.x * 1.f, root.y * 0.f, root.z * 1.f};
    Centred c;
    c.pos = qrot(q, V3{pos.x - xz.x, (pos.y - fl) - xz.y, pos.z - xz.z});
    c.vel = qrot(q, vel);
    if (j < 21) rot6d_roundtrip(d, c.rot);
    else {
#pragma unroll
        for (int k = 0; k < 6; ++k) c.rot[k] = 0.f;
    }
    return c;
}

__device__ __forceinline__ float ddim(float x, float x0, float c0, float c1, float c2, float c3) {
    const float eps = (c0 * x - x0) / c1;        // _predict_eps_from_xstart  gaussian_diffusion.py:558-562
    return x0 * c2 + c3 * eps;                   // eta = 0 mean             :1949-1956
}

// ---------------------------------------------------------------------------------------------------------
// Step noise of the stochastic DDIM family (eta > 0): Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
// keyed by the call's seed and counted by the element's own coordinates, so that an item's noise depends on neither B nor T.
// One definition for the update kernel and for the stateless fill (mmdm_randn_f32).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c[0]), l0 = 0xD2511F53u * c[0];
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u * c[2];
        c[0] = h1 ^ c[1] ^ k0; c[1] = l1; c[2] = h0 ^ c[3] ^ k1; c[3] = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// N(0, 1) of element (b, t, column) at loop position lp: counter (t * 524 + column, b, lp, 0), key (seed low, seed high); Box-Muller on
// u = ((r >> 8) + 0.5) 2^-24 of the first two words.  (k + 0.5 has 25 significant bits once k >= 2^23: there u1 is carried as its exact
// distance to one and the logarithm taken by log1pf, so the radius keeps its accuracy where it is small -- sqrt(2 (1 - u1)) near u1 = 1.)
__device__ __forceinline__ float step_normal(unsigned long long seed, int lp, int b, int t, int col) {
    uint32_t c[4] = {(uint32_t)(t * NF2 + col), (uint32_t)b, (uint32_t)lp, 0u};
    philox4x32_10(c, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
    const uint32_t a = c[0] >> 8, g = c[1] >> 8;
    const float lg = a < (1u << 23) ? logf(((float)a + 0.5f) * 0x1p-24f) : log1pf(-(((float)((1u << 24) - a) - 0.5f) * 0x1p-24f));
    const float u2 = ((float)g + 0.5f) * 0x1p-24f;
    return sqrtf(-2.0f * lg) * cosf(6.2831855f * u2);
}

__global__ __launch_bounds__(256) void randn_kernel(unsigned long long seed, int lp, int T, size_t total, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int col = (int)(idx % NF2);
    const size_t fr = idx / NF2;
    out[idx] = step_normal(seed, lp, (int)(fr / T), (int)(fr % T), col);
}

// what the NOISE forms of the update kernel take beside the plain form's arguments
struct NoiseArgs {
    const float* coef_eta;         // [2, S]: sqrt(1 - ab_prev - sigma^2), sigma
    const mmdm_opts_desc* od;      // the call's noise buffer / seed (device-side: a captured graph bakes in this address only)
    const int* loop_pos;
};
__device__ __forceinline__ const NoiseArgs& noise_args(const NoiseArgs& a) { return a; }

// NOISE: 0 = the deterministic update (eta = 0; no extra argument: NA is empty and the kernel is what it was before the forms 1 / 2 existed),
// 1 = + sigma * noise[loop_pos] from the caller's buffer [n_steps, B, T, 524], 2 = + sigma * step_normal(seed, loop_pos, ...).  Forms 1 / 2 read
// sqrt(1 - ab_prev - sigma^2) and sigma from the eta table and add no noise at i = 0 (gaussian_diffusion.py:1958-1963); the same noise goes to both chains.
// RAG forms 1 / 2: the buffer is packed [n_steps, sum(lens), 524] -- a slot's element is the chains' own index, the slot stride comes from the descriptor
// (it differs between batches that replay one graph) -- and the generator is keyed per item: (item_seed[b], item_noise_row[b]) stand for (seed, b), so that
// an item draws what it draws in the call it is meant to equal.  Padding rows have left by then.
template <bool RAG, int NOISE = 0, typename... NA>
__global__ __launch_bounds__(256) void xstart_ddim_kernel(const float* __restrict__ m, const float* __restrict__ stats, const float* __restrict__ coef,
                                                           int S, const int* __restrict__ step_idx, float* __restrict__ x, float* __restrict__ x2,
                                                           float* __restrict__ px1, float* __restrict__ px2, const float* __restrict__ floor_ws,
                                                           int B, int T, int align, mmdm_rag rg, NA... na) {
    static_assert(NOISE == 0 ? sizeof...(NA) == 0 : sizeof...(NA) == 1, "forms 1 / 2 take one NoiseArgs");
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    int j, t, p, b;
    size_t seq;
    if constexpr (RAG) {                         // thread = (frame row, person, joint) of the ragged batch (mixer_pre_kernel)
        if (idx >= rg.rows * 2 * NJ) return;
        j = idx % NJ;
        p = (idx / NJ) % 2;
        const int r = idx / (NJ * 2);
        b = rg.row_item[r];
        if (b < 0) return;
        t = rg.row_pos[r];
        seq = (size_t)(r - t) * NF2 + (size_t)p * NF;
    } else {
        const int total = B * 2 * T * NJ;
        if (idx >= total) return;
        j = idx % NJ;
        t = (idx / NJ) % T;
        p = (idx / (NJ * T)) % 2;
        b = idx / (NJ * T * 2);
        seq = (size_t)b * T * NF2 + (size_t)p * NF;
    }
    const int i = *step_idx;
    const float c0 = coef[i], c1 = coef[S + i], c2 = coef[2 * S + i];
    float c3, sigma = 0.f;
    int lp = 0, nb = b;                          // nb: the item's `b` in the generator's counter
    unsigned long long seed = 0;
    const float* nz = nullptr;
    if constexpr (NOISE == 0) c3 = coef[3 * S + i];
    else {
        const NoiseArgs& a = noise_args(na...);
        c3 = a.coef_eta[i];
        sigma = a.coef_eta[S + i];
        lp = *a.loop_pos;
        if constexpr (NOISE == 1 && RAG) nz = lp < a.od->noise_steps ? a.od->noise + (size_t)lp * (size_t)a.od->noise_stride : nullptr;
        else if constexpr (NOISE == 1) nz = lp < a.od->noise_steps ? a.od->noise + (size_t)lp * B * T * NF2 : nullptr;   // (the host refuses a run past the buffer)
        else if constexpr (RAG) { seed = a.od->item_seed[b]; nb = a.od->item_noise_row[b]; }
        else seed = a.od->seed;
    }
    const bool norm = i > 0;                                     // `if t[0] > 0`  gaussian_diffusion.py:2052
    const float* mh = stats, *sh = stats + NF, *mi = stats + 2 * NF, *si = stats + 3 * NF;
    const size_t off = seq + (size_t)t * NF2;
    const float* mo = m + off;

    // channels owned by this thread: pos j (3), vel j (3), rot j (6, j < 21) or feet (4, j == 21)
    float raw[12], v1[12];
    int ch[12];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ch[cnt] = 3 * j + k; ++cnt; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { ch[cnt] = 66 + 3 * j + k; ++cnt; }
    if (j < 21) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { ch[cnt] = ROT0 + 6 * j + k; ++cnt; }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { ch[cnt] = FEET0 + k; ++cnt; }
        ch[10] = 0; ch[11] = 0;
    }
    const int nch = (j < 21) ? 12 : 10;
#pragma unroll
    for (int k = 0; k < 12; ++k) { raw[k] = (k < nch) ? mo[ch[k]] : 0.f; v1[k] = raw[k]; }

    if (norm && align) {
        float d[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = raw[6 + k];
        const Centred c = center_channels(floor_ws[b * 2 + p], m + seq, j, V3{raw[0], raw[1], raw[2]}, V3{raw[3], raw[4], raw[5]}, d);
        v1[0] = c.pos.x; v1[1] = c.pos.y; v1[2] = c.pos.z;
        v1[3] = c.vel.x; v1[4] = c.vel.y; v1[5] = c.vel.z;
#pragma unroll
        for (int k = 0; k < 6; ++k) v1[6 + k] = c.rot[k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        if (k >= nch) continue;
        const int c = ch[k];
        float x0a = v1[k], x0b = raw[k];
        if (norm) {
            x0a = (x0a - mh[c]) / sh[c];
            x0b = (x0b - mi[c]) / si[c];
        }
        const size_t e = off + c;
        if constexpr (NOISE == 0) {
            x[e] = ddim(x[e], x0a, c0, c1, c2, c3);
            x2[e] = ddim(x2[e], x0b, c0, c1, c2, c3);
        } else {
            float va = ddim(x[e], x0a, c0, c1, c2, c3), vb = ddim(x2[e], x0b, c0, c1, c2, c3);
            if (i != 0) {                                        // nonzero_mask * sigma * noise, one draw for both chains   :1947, 1958-1963
                float z;
                if constexpr (NOISE == 1) z = nz ? nz[e] : 0.f;
                else z = step_normal(seed, lp, nb, t, p * NF + c);
                const float sn = sigma * z;
                va += sn; vb += sn;
            }
            x[e] = va;
            x2[e] = vb;
        }
        if (px1) px1[e] = x0a;
        if (px2) px2[e] = x0b;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Centring of the InterCLIP individual evaluator (EvaluatorModelWrapperIndividual, src/evaluation/utils.py:284-288): every person of every item becomes
// smpl_to_ih(center_motion(ih_to_smpl(person))) before it is encoded as a motion of its own.  motions [nitems, Tpad, npers * 262] with element strides.
// CONTRACT (the reference's, kept):
//   * the floor is the minimum of position Y over ALL Tpad frames handed in x 22 joints, not over the item's length: the reference centres the padded
//     buffer before it slices to the longest length, so a zero-padded tail contributes 0 to the minimum;
//   * frame 0 supplies the root XZ and the hip-across vector (joints 2, 1); the facing rotation is qbetween(normalize(cross(Y, across)), +Z);
//   * the cross product runs along the last dimension for EVERY batch size (the reference's torch.cross without dim goes wrong at a per-call batch of
//     exactly 3, SURVEY quirk 9: not reproduced);
//   * channels 258..261 of every person come out 0.
// Not pinned: fminf drops a NaN where torch.min propagates it; coincident hips divide by zero here as they do in the reference.
// Launch shape: a block per (item, person) for the floor, then one thread per (item, person, frame, joint) as in the update kernel -- HBM-bound, the
// 21 rotation round trips of a frame spread over lanes.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void center_floor_kernel(const float* __restrict__ m, long long item_stride, int row_stride, int Tpad, int npers,
                                                            float* __restrict__ floor_ws) {
    const int ip = blockIdx.x;                   // item * npers + person
    const float* base = m + (size_t)(ip / npers) * item_stride + (size_t)(ip % npers) * NF;
    float v = INFINITY;
    for (int i = threadIdx.x; i < Tpad * NJ; i += blockDim.x) {
        const int t = i / NJ, j = i % NJ;
        v = fminf(v, base[(size_t)t * row_stride + 3 * j + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) floor_ws[ip] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// joint j of frame `mo` (the person's 262 features of that frame) centred; the feet are not read: they come out 0 whatever they hold
__device__ __forceinline__ Centred center_joint(float fl, const float* f0, const float* __restrict__ mo, int j) {
    float d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = j < 21 ? mo[ROT0 + 6 * j + k] : 0.f;
    return center_channels(fl, f0, j, V3{mo[3 * j], mo[3 * j + 1], mo[3 * j + 2]}, V3{mo[66 + 3 * j], mo[66 + 3 * j + 1], mo[66 + 3 * j + 2]}, d);
}

// out[i, t, p * 262 + c] for all Tpad frames; one thread per (item, person, frame, joint)
__global__ __launch_bounds__(256) void center_motion_kernel(const float* __restrict__ m, long long item_stride, int row_stride, int Tpad, int npers,
                                                             long long total, float* __restrict__ out, long long out_item_stride, int out_row_stride,
                                                             const float* __restrict__ floor_ws) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % NJ);
    long long r = idx / NJ;
    const int t = (int)(r % Tpad);
    r /= Tpad;
    const int p = (int)(r % npers);
    const long long i = r / npers;
    const float* pb = m + (size_t)i * item_stride + (size_t)p * NF;          // frame 0 of the person
    const Centred c = center_joint(floor_ws[i * npers + p], pb, pb + (size_t)t * row_stride, j);
    float* o = out + (size_t)i * out_item_stride + (size_t)t * out_row_stride + (size_t)p * NF;
    o[3 * j] = c.pos.x; o[3 * j + 1] = c.pos.y; o[3 * j + 2] = c.pos.z;
    o[66 + 3 * j] = c.vel.x; o[66 + 3 * j + 1] = c.vel.y; o[66 + 3 * j + 2] = c.vel.z;
    if (j < 21) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[ROT0 + 6 * j + k] = c.rot[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[FEET0 + k] = c.rot[k];
    }
}

// The same values written straight into the embedding GEMM's A operand of the ragged motion encoder (rowops.hip motion_pack_kernel with npers = 1 on the
// centred motion): sequence s = 2 * item + person owns rows [seq_off[s], seq_off[s] + seq_len[s]) -- the token row (zeros), then its first
// seq_len[s] - 1 frames, 258 centred channels each, columns [258, Kp) zeros.  32 threads per row, 8 rows per block: lanes 0..21 are the joints, the other
// ten write the zero columns.  Frames at and beyond the length are never transformed or written (only their position Y is read, by the floor); rows
// outside every sequence are not touched.
// SPLIT: the same elements as the two fp16 planes of the fp32-split embedding GEMM's A operand ([2][total_rows][lda], plane stride in elements) instead of
// fp32 rows -- each value is formed exactly as in the fp32 form and split on its way out (kernels.h mmdm_split2), a zero is +0 in both planes.
template <bool SPLIT>
__device__ __forceinline__ void pack_store(void* __restrict__ A, size_t plane, size_t i, float v) {
    if constexpr (SPLIT) {
        _Float16 hi, lo;
        mmdm_split2(v, hi, lo);
        static_cast<_Float16*>(A)[i] = hi;
        static_cast<_Float16*>(A)[plane + i] = lo;
    } else {
        static_cast<float*>(A)[i] = v;
    }
}

template <bool SPLIT>
__global__ __launch_bounds__(256) void center_pack_kernel(const float* __restrict__ m, long long item_stride, int row_stride, int Tpad,
                                                           void* __restrict__ A, size_t plane, int lda, int Kp, const int* __restrict__ seq_off,
                                                           const int* __restrict__ seq_len, int total_rows, const float* __restrict__ floor_ws) {
    const int s = blockIdx.y, pos = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    if (pos >= seq_len[s] || pos > Tpad) return;
    const long long row = (long long)seq_off[s] + pos;
    if (row < 0 || row >= total_rows) return;
    const size_t r0 = (size_t)row * lda;
    if (pos == 0) {
        for (int c = l; c < Kp; c += 32) pack_store<SPLIT>(A, plane, r0 + c, 0.f);
        return;
    }
    if (l >= NJ) {
        for (int c = FEET0 + (l - NJ); c < Kp; c += 32 - NJ) pack_store<SPLIT>(A, plane, r0 + c, 0.f);
        return;
    }
    const float* pb = m + (size_t)(s >> 1) * item_stride + (size_t)(s & 1) * NF;
    const Centred c = center_joint(floor_ws[s], pb, pb + (size_t)(pos - 1) * row_stride, l);
    pack_store<SPLIT>(A, plane, r0 + 3 * l, c.pos.x); pack_store<SPLIT>(A, plane, r0 + 3 * l + 1, c.pos.y); pack_store<SPLIT>(A, plane, r0 + 3 * l + 2, c.pos.z);
    pack_store<SPLIT>(A, plane, r0 + 66 + 3 * l, c.vel.x); pack_store<SPLIT>(A, plane, r0 + 66 + 3 * l + 1, c.vel.y); pack_store<SPLIT>(A, plane, r0 + 66 + 3 * l + 2, c.vel.z);
    if (l < 21) {
#pragma unroll
        for (int k = 0; k < 6; ++k) pack_store<SPLIT>(A, plane, r0 + ROT0 + 6 * l + k, c.rot[k]);
    }
}

// ClassifierFreeSampleModel combine + single-chain DDIM update on rows of any width C (262: one person, 524: two).  The forms of xstart_ddim_kernel:
// NOISE 0 = the deterministic update (no extra argument: the kernel the single-chain samplers have always launched), 1 = + sigma * noise[loop_pos] from the
// caller's buffer [n_steps, per_batch_total], 2 = + sigma * step_normal(seed, loop_pos, b, t, column) -- the generator's counter is (t * 524 + column, b, lp)
// whatever C is, so what mmdm_randn_f32 writes is what a 524-wide chain draws.  Forms 1 / 2 take sqrt(1 - ab_prev - sigma^2) and sigma from the eta table
// and add no noise at i = 0 (gaussian_diffusion.py:840-848).  RAG: the chain is a group of rg.rows frame rows (padding rows return: they stay zero), the
// uncond half of m lies per_batch_total = rg.rows * C further on, a slot of the packed noise buffer is noise_stride elements (descriptor) and the generator is
// keyed per item by (item_seed[b], item_noise_row[b]).
struct CfgRows { int T, C; mmdm_rag rg; };          // what every form but <false, 0> takes beside the plain arguments: the rows' coordinates
__device__ __forceinline__ const CfgRows& cfg_rows_of(const CfgRows& r) { return r; }
__device__ __forceinline__ const CfgRows& cfg_rows_of(const CfgRows& r, const NoiseArgs&) { return r; }
__device__ __forceinline__ const NoiseArgs& cfg_noise_of(const CfgRows&, const NoiseArgs& a) { return a; }
template <bool RAG = false, int NOISE = 0, typename... NA>
__global__ __launch_bounds__(256) void cfg_ddim_kernel(const float* __restrict__ m, const float* __restrict__ coef, int S, const int* __restrict__ step_idx,
                                                        float s, float* __restrict__ x, float* __restrict__ px, size_t per_batch_total, NA... na) {
    static_assert((!RAG && NOISE == 0) ? sizeof...(NA) == 0 : (NOISE == 0 ? sizeof...(NA) == 1 : sizeof...(NA) == 2), "forms: (), (CfgRows), (CfgRows, NoiseArgs)");
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per_batch_total) return;
    const int i = *step_idx;
    if constexpr (!RAG && NOISE == 0) {
        const float x0 = s * m[idx] + (1.0f - s) * m[per_batch_total + idx];   // cfg_sampler.py:24-28
        x[idx] = ddim(x[idx], x0, coef[i], coef[S + i], coef[2 * S + i], coef[3 * S + i]);
        if (px) px[idx] = x0;
    } else {
        const CfgRows& cr = cfg_rows_of(na...);
        const int col = (int)(idx % cr.C);
        const size_t fr = idx / cr.C;
        int b, t;
        if constexpr (RAG) {
            b = cr.rg.row_item[fr];
            if (b < 0) return;
            t = cr.rg.row_pos[fr];
        } else {
            b = (int)(fr / cr.T);
            t = (int)(fr % cr.T);
        }
        const float x0 = s * m[idx] + (1.0f - s) * m[per_batch_total + idx];
        if constexpr (NOISE == 0) {
            x[idx] = ddim(x[idx], x0, coef[i], coef[S + i], coef[2 * S + i], coef[3 * S + i]);
        } else {
            const NoiseArgs& a = cfg_noise_of(na...);
            float v = ddim(x[idx], x0, coef[i], coef[S + i], coef[2 * S + i], a.coef_eta[i]);
            if (i != 0) {                                        // nonzero_mask * sigma * noise
                const int lp = *a.loop_pos;
                float z;
                if constexpr (NOISE == 1) {
                    const size_t stride = RAG ? (size_t)a.od->noise_stride : per_batch_total;
                    z = lp < a.od->noise_steps ? a.od->noise[(size_t)lp * stride + idx] : 0.f;       // (the host refuses a run past the buffer)
                } else if constexpr (RAG) z = step_normal(a.od->item_seed[b], lp, a.od->item_noise_row[b], t, col);
                else z = step_normal(a.od->seed, lp, b, t, col);
                v = __builtin_fmaf(a.coef_eta[S + i], z, v);     // (one fixed operation: every instantiation rounds alike)
            }
            x[idx] = v;
        }
        if (px) px[idx] = x0;
    }
}

// The same update behind the other two guidance wrappers: x0 = the wrapper's combine at element idx (a functor: its expression keeps its operation order in
// every form), then exactly cfg_ddim_kernel's forms -- <false, 0> is the kernel the stand-alone 4-way CFG and dual samplers (single_only 2 / 3) have always
// launched, the others serve single_only = 4 with cfg_form 1 / 2 (the loop's options, ragged groups: the further CFG copies of the model output lie
// per_batch_total = rg.rows * C apart).
template <bool RAG, int NOISE, typename X0, typename... NA>
__device__ __forceinline__ void combine_ddim(const X0& x0_of, const float* __restrict__ coef, int S, const int* __restrict__ step_idx, float* __restrict__ x,
                                             float* __restrict__ px, size_t per_batch_total, NA... na) {
    static_assert((!RAG && NOISE == 0) ? sizeof...(NA) == 0 : (NOISE == 0 ? sizeof...(NA) == 1 : sizeof...(NA) == 2), "forms: (), (CfgRows), (CfgRows, NoiseArgs)");
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per_batch_total) return;
    const int i = *step_idx;
    if constexpr (!RAG && NOISE == 0) {
        const float x0 = x0_of(idx, i);
        x[idx] = ddim(x[idx], x0, coef[i], coef[S + i], coef[2 * S + i], coef[3 * S + i]);
        if (px) px[idx] = x0;
    } else {
        const CfgRows& cr = cfg_rows_of(na...);
        const int col = (int)(idx % cr.C);
        const size_t fr = idx / cr.C;
        int b, t;
        if constexpr (RAG) {
            b = cr.rg.row_item[fr];
            if (b < 0) return;
            t = cr.rg.row_pos[fr];
        } else {
            b = (int)(fr / cr.T);
            t = (int)(fr % cr.T);
        }
        const float x0 = x0_of(idx, i);
        if constexpr (NOISE == 0) {
            x[idx] = ddim(x[idx], x0, coef[i], coef[S + i], coef[2 * S + i], coef[3 * S + i]);
        } else {
            const NoiseArgs& a = cfg_noise_of(na...);
            float v = ddim(x[idx], x0, coef[i], coef[S + i], coef[2 * S + i], a.coef_eta[i]);
            if (i != 0) {                                        // nonzero_mask * sigma * noise
                const int lp = *a.loop_pos;
                float z;
                if constexpr (NOISE == 1) {
                    const size_t stride = RAG ? (size_t)a.od->noise_stride : per_batch_total;
                    z = lp < a.od->noise_steps ? a.od->noise[(size_t)lp * stride + idx] : 0.f;       // (the host refuses a run past the buffer)
                } else if constexpr (RAG) z = step_normal(a.od->item_seed[b], lp, a.od->item_noise_row[b], t, col);
                else z = step_normal(a.od->seed, lp, b, t, col);
                v = __builtin_fmaf(a.coef_eta[S + i], z, v);     // (one fixed operation: every instantiation rounds alike)
            }
            x[idx] = v;
        }
        if (px) px[idx] = x0;
    }
}

// ClassifierFreeSampleModelMultiple: (s*full) + (s_int*interaction-only) + (s_ind*individuals-only) + ((1-(s+s_int+s_ind))*uncond)   cfg_sampler.py:97
struct Cfg4X0 {
    const float* __restrict__ m; float s, si, sd; size_t per_batch_total;
    __device__ __forceinline__ float operator()(size_t idx, int) const {
        return (s * m[idx]) + (si * m[per_batch_total + idx]) + (sd * m[2 * per_batch_total + idx]) + ((1.0f - (s + si + sd)) * m[3 * per_batch_total + idx]);
    }
};
template <bool RAG = false, int NOISE = 0, typename... NA>
__global__ __launch_bounds__(256) void cfg4_ddim_kernel(const float* __restrict__ m, const float* __restrict__ coef, int S, const int* __restrict__ step_idx,
                                                         float s, float si, float sd, float* __restrict__ x, float* __restrict__ px, size_t per_batch_total,
                                                         NA... na) {
    combine_ddim<RAG, NOISE>(Cfg4X0{m, s, si, sd, per_batch_total}, coef, S, step_idx, x, px, per_batch_total, na...);
}

// ClassifierFreeSampleDualMDM.forward combine (cfg_sampler.py:139-150) + DDIM update: per-model guidance, then the
// time-scheduled blend out_int + w[step] (out_ind - out_int).
struct DualX0 {
    const float* __restrict__ mi; const float* __restrict__ mI; const float* __restrict__ wtab; float s_ind, s_int; size_t per_batch_total;
    __device__ __forceinline__ float operator()(size_t idx, int i) const {
        const float ui = mi[per_batch_total + idx], uI = mI[per_batch_total + idx];
        const float gI = uI + s_int * (mI[idx] - uI);
        const float gi = ui + s_ind * (mi[idx] - ui);
        return gI + wtab[i] * (gi - gI);
    }
};
template <bool RAG = false, int NOISE = 0, typename... NA>
__global__ __launch_bounds__(256) void dual_ddim_kernel(const float* __restrict__ mi, const float* __restrict__ mI, const float* __restrict__ coef, int S,
                                                         const int* __restrict__ step_idx, const float* __restrict__ wtab, float s_ind, float s_int,
                                                         float* __restrict__ x, float* __restrict__ px, size_t per_batch_total, NA... na) {
    combine_ddim<RAG, NOISE>(DualX0{mi, mI, wtab, s_ind, s_int, per_batch_total}, coef, S, step_idx, x, px, per_batch_total, na...);
}

// The REVERSE update of the one-chain samplers (GaussianDiffusion.ddim_reverse_sample, gaussian_diffusion.py:932-944): the deterministic ODE taken upwards,
//   eps = (c_recip[i] x - x0) / c_recipm1[i];   x = x0 sqrt(ab_next[i]) + sqrt(1 - ab_next[i]) eps
// -- the same ddim() with rows 2 / 3 of the coefficient table replaced by the rows of rev [2, S], so a reverse update rounds as a forward update does.  x0 is
// the step's pred_xstart as the forward step's combine kernel left it (any guidance wrapper).  No noise forms: the reference asserts eta == 0.  Rows of any
// width C; RAG: row_item [rows] of the group, padding rows (row_item < 0) are left untouched.
template <bool RAG>
__global__ __launch_bounds__(256) void ddim_reverse_kernel(const float* __restrict__ x0, const float* __restrict__ coef, const float* __restrict__ rev, int S,
                                                            const int* __restrict__ step_idx, float* __restrict__ x, size_t total,
                                                            const int* __restrict__ row_item, int C) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    if constexpr (RAG) {
        if (row_item[idx / C] < 0) return;
    }
    const int i = *step_idx;
    x[idx] = ddim(x[idx], x0[idx], coef[i], coef[S + i], rev[i], rev[S + i]);
}

__global__ void step_dec_kernel(int* step_idx, int* loop_pos) { *step_idx -= 1; *loop_pos += 1; }
__global__ void set_step_kernel(int* step_idx, int* loop_pos, int s, int l) { *step_idx = s; *loop_pos = l; }

// x_start of the loop (gaussian_diffusion.py:1877-1882): the ground path of both persons' roots -- columns 0, 2, 262, 264 -- of both chains is
// overwritten with x_start[:, :T] before the models run.  x_start [B, xs_T >= T, 524] comes from the call's device-side descriptor.
// TWO = false: the one-chain form (the stand-alone InterGen sampler: one 524-wide chain, x2 unused).
template <bool TWO = true>
__global__ __launch_bounds__(256) void pin_root_kernel(float* __restrict__ x, float* __restrict__ x2, const mmdm_opts_desc* __restrict__ od, int B, int T) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * T * 4) return;
    const float* xs = od->x_start;
    const int xs_T = od->xs_T;
    if (!xs || xs_T < T) return;
    const int k = idx & 3, fr = idx >> 2;
    const int col = (k >> 1) * NF + (k & 1) * 2;
    const int b = fr / T, t = fr % T;
    const float v = xs[((size_t)b * xs_T + t) * NF2 + col];
    const size_t e = (size_t)fr * NF2 + col;
    x[e] = v;
    if constexpr (TWO) x2[e] = v;
}

// ragged form: one thread per (frame row of the group, pinned column); x_start is packed [sum(lens), 524] like x_T, padding rows are never looked up
template <bool TWO = true>
__global__ __launch_bounds__(256) void pin_root_rag_kernel(float* __restrict__ x, float* __restrict__ x2, const mmdm_opts_desc* __restrict__ od, mmdm_rag rg) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rg.rows * 4) return;
    const float* xs = od->x_start;
    if (!xs) return;
    const int k = idx & 3, r = idx >> 2;
    if (rg.row_item[r] < 0) return;
    const size_t e = (size_t)r * NF2 + (k >> 1) * NF + (k & 1) * 2;
    const float v = xs[e];
    x[e] = v;
    if constexpr (TWO) x2[e] = v;
}

// q_sample at the start of a call (gaussian_diffusion.py:1859-1863, 465-485): x = a * init + b * x_T on both chains (init == nullptr: zeros)
// TWO = false: one chain of any width (gaussian_diffusion.py:1036-1045)
template <bool TWO = true>
__global__ __launch_bounds__(256) void q_sample_kernel(float* __restrict__ x, float* __restrict__ x2, const float* __restrict__ init, float a, float b, size_t total) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const float v = a * (init ? init[idx] : 0.f) + b * x[idx];
    x[idx] = v;
    if constexpr (TWO) x2[idx] = v;
}

__global__ void set_opts_kernel(mmdm_opts_desc* d, mmdm_opts_desc v) { *d = v; }

struct RagItemNoise { unsigned long long seed[MMDM_RAG_MAX_ITEMS]; int row[MMDM_RAG_MAX_ITEMS]; };
__global__ __launch_bounds__(256) void set_item_noise_kernel(RagItemNoise v, int B, unsigned long long* __restrict__ item_seed, int* __restrict__ item_noise_row) {
    const int b = threadIdx.x;
    if (b >= B) return;
    item_seed[b] = v.seed[b];
    item_noise_row[b] = v.row[b];
}

// which: 0 -> hd->o1, 1 -> hd->o2; a null destination (history not requested for this call) makes the launch a no-op
__global__ void hist_copy_kernel(const float* __restrict__ src, const mmdm_hist_desc* __restrict__ hd, int which, size_t count, const int* __restrict__ loop_pos) {
    float* dst = which ? hd->o2 : hd->o1;
    if (!dst) return;
    const long slot = hist_slot(loop_pos, hd->every);
    if (slot < 0) return;
    float* d = dst + (size_t)slot * count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) d[i] = src[i];
}

// Pose rows -> 16-byte-aligned, zero-padded GEMM operands: dst[p][r][0:ldp] = (src[r][p*262 : p*262+262], 0 ...).  The 262-float person
// slices of a [rows, 524] motion tensor start at byte 1048 (not 16-byte aligned) and 262 is not a multiple of the GEMM's K step, so
// the embedding GEMMs would otherwise run on the register-staged fallback kernel.
__global__ void repack_pose_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int npers, int rows, int ldp) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)rows * ldp;
    if (i >= per * npers) return;
    const int p = (int)(i / per);
    const size_t rem = i - (size_t)p * per;
    const size_t r = rem / ldp;
    const int c = (int)(rem - r * ldp);
    dst[i] = c < MMDM_NF ? src[r * ld_src + (size_t)p * MMDM_NF + c] : 0.f;
}

// the same rows as the two fp16 planes of the fp32-split GEMM (kernels.h mmdm_split2): dst [npers][2][rows][ldp]
__global__ void repack_pose_split_kernel(const float* __restrict__ src, int ld_src, _Float16* __restrict__ dst, int npers, int rows, int ldp) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)rows * ldp;
    if (i >= per * npers) return;
    const int p = (int)(i / per);
    const size_t rem = i - (size_t)p * per;
    const size_t r = rem / ldp;
    const int c = (int)(rem - r * ldp);
    const float x = c < MMDM_NF ? src[r * ld_src + (size_t)p * MMDM_NF + c] : 0.f;
    _Float16 h, l;
    mmdm_split2(x, h, l);
    dst[(size_t)p * 2 * per + rem] = h;
    dst[(size_t)p * 2 * per + per + rem] = l;
}

__global__ void gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ idx, float* __restrict__ dst, int n, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * D) return;
    dst[i] = src[(size_t)idx[i / D] * D + (i % D)];
}

}  // namespace

// One launcher per kernel: the rows of the call are an argument (kernels.h mmdm_rows -- uniform, or a ragged batch's row maps), the stateless entry
// points of include/mmdm.h check their arguments and pass {n, T}.
// ragged batch: r.n / fr->B groups of fr->rows frame rows (the cond | uncond halves of the CFG-doubled batch)
int mmdm_mixer_pre(const float* o1, const float* o2, const float* stats, float* out1, float* out2, const mmdm_rows& r, int align, const int* last_frame,
                   int last_rows, hipStream_t st) {
    if (r.fr) {
        const int groups = r.n / r.fr->B, total = groups * r.fr->rows * 2 * MMDM_NJ;
        hipLaunchKernelGGL(mixer_pre_kernel<true>, dim3((total + 255) / 256), dim3(256), 0, st, o1, o2, stats, out1, out2, groups, 0, align, *r.fr, (const int*)nullptr, 1);
        return mmdm_check_launch("mixer_pre_rag");
    }
    const int total = r.n * 2 * r.T * MMDM_NJ;
    hipLaunchKernelGGL(mixer_pre_kernel<false>, dim3((total + 255) / 256), dim3(256), 0, st, o1, o2, stats, out1, out2, r.n, r.T, align, mmdm_rag{}, last_frame,
                       last_frame ? last_rows : 1);
    return mmdm_check_launch("mixer_pre");
}

extern "C" int mmdm_mixer_pre_f32(const float* o1, const float* o2, const float* stats, float* out1, float* out2,
                                  int n, int T, int align, void* stream) {
    if (n == 0 || T == 0) return MMDM_OK;
    if (!o1 || !o2 || !stats || !out1 || !out2 || n < 0 || T < 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_mixer_pre_f32: bad arguments");
    return mmdm_mixer_pre(o1, o2, stats, out1, out2, mmdm_rows{n, T}, align, nullptr, 0, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_mixer_pre_masked_f32(const float* o1, const float* o2, const float* stats, float* out1, float* out2,
                                         int n, int T, int align, const int* last_frame, int last_rows, void* stream) {
    if (n == 0 || T == 0) return MMDM_OK;
    if (!o1 || !o2 || !stats || !out1 || !out2 || n < 0 || T < 0 || (last_frame && last_rows <= 0)) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_mixer_pre_masked_f32: bad arguments");
    return mmdm_mixer_pre(o1, o2, stats, out1, out2, mmdm_rows{n, T}, align, last_frame, last_rows, static_cast<hipStream_t>(stream));
}

// hd != null: the history destinations are read from the device-side descriptor and the slot is chosen on the device (graph replay): see hist_slot().
// Influence history rows are then [.., 262] for modes 3-4 and [.., 1] for modes 1-2 (the reference's shapes).  Ragged batch: history slots are
// [2 * fr->rows, C] (padding rows are never written), and only "per frame" vs "per sequence" of Tw matters.
int mmdm_blend_cfg(const float* out1, const float* out2, const float* w, int mode, int use_force, float force, float cfg_scale, float* model_out,
                   float* hist_i1, float* hist_i2, float* hist_mix, const mmdm_hist_desc* hd, const int* loop_pos, const mmdm_rows& r, hipStream_t st) {
    if (mode < 1 || mode > 4) return mmdm_set_error(MMDM_ERR_ARG, "Mixing mode not recognized");   // mixermdm.py:786
    const bool per_frame = mode == 2 || mode == 4;
    const int nw = (mode >= 3) ? 23 : 1, nwh = hd && mode < 3 ? 1 : MMDM_NF;
    if (r.fr) {
        const size_t total = (size_t)r.fr->rows * NF2;
        hipLaunchKernelGGL(blend_cfg_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out1, out2, w, per_frame ? 2 : 1, nw, use_force, force,
                           cfg_scale, model_out, hist_i1, hist_i2, hist_mix, hd, loop_pos, nwh, r.fr->B, 0, *r.fr);
        return mmdm_check_launch("blend_cfg_rag");
    }
    const size_t total = (size_t)r.n * r.T * NF2;
    hipLaunchKernelGGL(blend_cfg_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out1, out2, w, per_frame ? r.T : 1, nw, use_force, force,
                       cfg_scale, model_out, hist_i1, hist_i2, hist_mix, hd, loop_pos, nwh, r.n, r.T, mmdm_rag{});
    return mmdm_check_launch("blend_cfg");
}

extern "C" int mmdm_blend_cfg_f32(const float* out1, const float* out2, const float* w, int mode, int use_force, float force,
                                  float cfg_scale, float* model_out, float* hist_i1, float* hist_i2, float* hist_mix,
                                  int B, int T, void* stream) {
    if (B == 0 || T == 0) return MMDM_OK;
    if (!out1 || !out2 || !w || !model_out || B < 0 || T < 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_blend_cfg_f32: bad arguments");
    return mmdm_blend_cfg(out1, out2, w, mode, use_force, force, cfg_scale, model_out, hist_i1, hist_i2, hist_mix, nullptr, nullptr, mmdm_rows{B, T},
                          static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------------------------------------------------
// Ragged batches: the row maps of one sampling call, built ON THE DEVICE from the item lengths (passed by value: no host buffer to keep
// alive, no synchronisation) -- item offsets / lengths, item and frame index of every frame row of a group (-1 / 0 for the padding rows
// between the sum of lengths and the group stride `rows`), and per sequence of the `groups` x B sequences its first row and length.
// The MDM denoiser's TOKEN rows (one conditioning token in front of every item's frames) are a second set of maps from the same kernel: lengths + 1,
// the token stride as `rows`; row_pos 0 is then the token and k >= 1 frame k - 1.  row_seq and item_order may be null (no AdaLN lookup in that stack; the
// length order of the tokens is the frames').
// ---------------------------------------------------------------------------------------------------------
struct RagLens { int v[MMDM_RAG_MAX_ITEMS]; };
__global__ __launch_bounds__(256) void rag_setup_kernel(RagLens L, int B, int rows, int groups, int* __restrict__ item_off, int* __restrict__ item_len,
                                                        int* __restrict__ row_item, int* __restrict__ row_pos, int* __restrict__ row_seq,
                                                        int* __restrict__ seq_off, int* __restrict__ seq_len, int* __restrict__ item_order) {
    __shared__ int off[MMDM_RAG_MAX_ITEMS + 1];
    if (threadIdx.x == 0) {
        int a = 0;
        for (int b = 0; b < B; ++b) { off[b] = a; a += L.v[b]; }
        off[B] = a;
    }
    __syncthreads();
    const int RT = off[B];
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (int r = tid; r < groups * rows; r += nth) {
        const int g = r / rows, rl = r % rows;
        int item = -1, pos = 0;
        if (rl < RT) {
            int lo = 0, hi = B - 1;                       // largest b with off[b] <= rl
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= rl) lo = mid; else hi = mid - 1; }
            item = lo; pos = rl - off[lo];
        }
        if (g == 0) { row_item[rl] = item; row_pos[rl] = pos; }
        if (row_seq) row_seq[r] = g * B + (item < 0 ? 0 : item);
    }
    for (int s = tid; s < groups * B; s += nth) { seq_off[s] = (s / B) * rows + off[s % B]; seq_len[s] = L.v[s % B]; }
    for (int b = tid; b < B; b += nth) { item_off[b] = off[b]; item_len[b] = L.v[b]; }
    // items by length, longest first (ties in index order): item b's rank = the number of items that come before it (B <= 256: a rank sort by one block)
    if (blockIdx.x == 0 && item_order) {
        for (int b = threadIdx.x; b < B; b += blockDim.x) {
            int rank = 0;
            for (int c = 0; c < B; ++c) rank += (L.v[c] > L.v[b] || (L.v[c] == L.v[b] && c < b)) ? 1 : 0;
            item_order[rank] = b;
        }
    }
}

int mmdm_rag_setup(const int* lens_host, int B, int rows, int groups, int* item_off, int* item_len, int* row_item, int* row_pos, int* row_seq,
                   int* seq_off, int* seq_len, int* item_order, hipStream_t st) {
    if (B <= 0 || B > MMDM_RAG_MAX_ITEMS) return mmdm_set_error(MMDM_ERR_ARG, "ragged batch: %d items (1 .. %d)", B, MMDM_RAG_MAX_ITEMS);
    RagLens L;
    for (int b = 0; b < MMDM_RAG_MAX_ITEMS; ++b) L.v[b] = b < B ? lens_host[b] : 0;
    hipLaunchKernelGGL(rag_setup_kernel, dim3(64), dim3(256), 0, st, L, B, rows, groups, item_off, item_len, row_item, row_pos, row_seq, seq_off, seq_len, item_order);
    return mmdm_check_launch("rag_setup");
}

int mmdm_hist_copy(const float* src, const mmdm_hist_desc* hd, int which, size_t count, const int* loop_pos, hipStream_t st) {
    hipLaunchKernelGGL(hist_copy_kernel, dim3(1024), dim3(256), 0, st, src, hd, which, count, loop_pos);
    return mmdm_check_launch("hist_copy");
}

__global__ void set_hist_kernel(mmdm_hist_desc* d, mmdm_hist_desc v) { *d = v; }

int mmdm_set_hist_desc(mmdm_hist_desc* d, const mmdm_hist_desc& v, hipStream_t st) {
    hipLaunchKernelGGL(set_hist_kernel, dim3(1), dim3(1), 0, st, d, v);
    return mmdm_check_launch("set_hist");
}

int mmdm_set_step(int* step_idx, int* loop_pos, int s, int l, hipStream_t st) {
    hipLaunchKernelGGL(set_step_kernel, dim3(1), dim3(1), 0, st, step_idx, loop_pos, s, l);
    return mmdm_check_launch("set_step");
}

int mmdm_gather_rows(const float* src, const int* idx, float* dst, int n, int D, hipStream_t st) {
    const size_t total = (size_t)n * D;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, idx, dst, n, D);
    return mmdm_check_launch("gather_rows");
}

// floor (when the update aligns) + the update, both in the instantiation of the call's rows and noise form; uniform: (B, T), ragged: (rg.B, 0) and the maps
template <bool RAG>
static int xstart_ddim_launch(int form, const float* model_out, const float* stats, const float* coef, int S, const int* step_idx, const NoiseArgs& na, float* x,
                              float* x2, float* pred_xstart, float* pred_xstart2, float* floor_ws, int B, int T, int total, int align, const mmdm_rag& rg,
                              hipStream_t st) {
    if (align) {
        hipLaunchKernelGGL(floor_kernel<RAG>, dim3(B * 2), dim3(256), 0, st, model_out, floor_ws, T, rg);
        if (int rc = mmdm_check_launch(RAG ? "floor_rag" : "floor")) return rc;
    }
    const dim3 grid((total + 255) / 256), block(256);
    if (form == 0)
        hipLaunchKernelGGL(xstart_ddim_kernel<RAG>, grid, block, 0, st, model_out, stats, coef, S, step_idx, x, x2, pred_xstart, pred_xstart2, floor_ws, B, T, align, rg);
    else if (form == 1)
        hipLaunchKernelGGL((xstart_ddim_kernel<RAG, 1, NoiseArgs>), grid, block, 0, st, model_out, stats, coef, S, step_idx, x, x2, pred_xstart, pred_xstart2, floor_ws,
                           B, T, align, rg, na);
    else
        hipLaunchKernelGGL((xstart_ddim_kernel<RAG, 2, NoiseArgs>), grid, block, 0, st, model_out, stats, coef, S, step_idx, x, x2, pred_xstart, pred_xstart2, floor_ws,
                           B, T, align, rg, na);
    return mmdm_check_launch(RAG ? "xstart_ddim_rag" : "xstart_ddim");
}

// the update of both chains: form 0 deterministic, 1 / 2 with step noise (the caller's buffer / the device generator; ragged: the packed buffer / the
// generator keyed per item).  Ragged batch (fr->B items, fr->rows frame rows incl. padding): same arithmetic per item
int mmdm_xstart_ddim(int form, const float* model_out, const float* stats, const float* coef, const float* coef_eta, int S, const int* step_idx,
                     const int* loop_pos, const mmdm_opts_desc* od, float* x, float* x2, float* pred_xstart, float* pred_xstart2, float* floor_ws,
                     const mmdm_rows& r, int align, hipStream_t st) {
    if (form < 0 || form > 2) return mmdm_set_error(MMDM_ERR_ARG, "xstart_ddim: form %d", form);
    const NoiseArgs na{coef_eta, od, loop_pos};
    if (r.fr)
        return xstart_ddim_launch<true>(form, model_out, stats, coef, S, step_idx, na, x, x2, pred_xstart, pred_xstart2, floor_ws, r.fr->B, 0,
                                        r.fr->rows * 2 * MMDM_NJ, align, *r.fr, st);
    return xstart_ddim_launch<false>(form, model_out, stats, coef, S, step_idx, na, x, x2, pred_xstart, pred_xstart2, floor_ws, r.n, r.T, r.n * 2 * r.T * MMDM_NJ,
                                     align, mmdm_rag{}, st);
}

extern "C" int mmdm_xstart_ddim_f32(const float* model_out, const float* stats, const float* coef, int S, const int* step_idx,
                                    float* x, float* x2, float* pred_xstart, float* pred_xstart2, float* floor_ws,
                                    int B, int T, int align, void* stream) {
    if (B == 0 || T == 0) return MMDM_OK;
    if (!model_out || !stats || !coef || !step_idx || !x || !x2 || !floor_ws || S <= 0 || B < 0 || T < 0)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_xstart_ddim_f32: bad arguments");
    return mmdm_xstart_ddim(0, model_out, stats, coef, nullptr, S, step_idx, nullptr, nullptr, x, x2, pred_xstart, pred_xstart2, floor_ws, mmdm_rows{B, T}, align,
                            static_cast<hipStream_t>(stream));
}

// what the two centring entries ask of their motions argument
static int center_args_check(const char* who, const float* motions, int64_t item_stride, int row_stride, int Tpad, int nitems, int npers, const float* floor_ws) {
    if (!motions || !floor_ws || nitems < 0 || npers < 1 || npers > 2 || Tpad < 0 || Tpad > (1 << 24) || row_stride < npers * MMDM_NF ||
        item_stride < (int64_t)Tpad * row_stride)
        return mmdm_set_error(MMDM_ERR_ARG, "%s: bad arguments nitems=%d npers=%d Tpad=%d row stride=%d item stride=%lld", who, nitems, npers, Tpad, row_stride,
                              (long long)item_stride);
    return MMDM_OK;
}

extern "C" int mmdm_center_motion_f32(const float* motions, int64_t item_stride, int row_stride, int Tpad, int nitems, int npers, float* out,
                                      int64_t out_item_stride, int out_row_stride, float* floor_ws, void* stream) {
    if (nitems == 0 || Tpad == 0) return MMDM_OK;
    if (int rc = center_args_check("mmdm_center_motion_f32", motions, item_stride, row_stride, Tpad, nitems, npers, floor_ws)) return rc;
    if (!out || out_row_stride < npers * MMDM_NF || out_item_stride < (int64_t)Tpad * out_row_stride)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_center_motion_f32: bad output row stride=%d item stride=%lld", out_row_stride, (long long)out_item_stride);
    if (out < motions + (int64_t)nitems * item_stride && motions < out + (int64_t)nitems * out_item_stride)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_center_motion_f32: the output must not alias the input (every frame reads frame 0 and the floor of its item)");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(center_floor_kernel, dim3(nitems * npers), dim3(256), 0, st, motions, (long long)item_stride, row_stride, Tpad, npers, floor_ws);
    if (int rc = mmdm_check_launch("center_floor")) return rc;
    const long long total = (long long)nitems * npers * Tpad * MMDM_NJ;
    if ((total + 255) / 256 > 0x7fffffffLL) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_center_motion_f32: %d items of %d frames exceed one launch", nitems, Tpad);
    hipLaunchKernelGGL(center_motion_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, motions, (long long)item_stride, row_stride, Tpad, npers, total,
                       out, (long long)out_item_stride, out_row_stride, floor_ws);
    return mmdm_check_launch("center_motion");
}

// planes != null: the operand as two fp16 planes (mmdm_center_pack_split) instead of the fp32 rows A; exactly one is given
static int center_pack(const char* who, const float* motions, int64_t item_stride, int row_stride, int Tpad, int nitems, float* A, void* planes, int64_t plane_stride,
                       int lda, int Kp, const int* seq_off, const int* seq_len, int max_len, int total_rows, float* floor_ws, void* stream) {
    if (nitems == 0) return MMDM_OK;
    if (int rc = center_args_check(who, motions, item_stride, row_stride, Tpad, nitems, 2, floor_ws)) return rc;
    // the sequence description of mmdm_rowop_motion_pack, two sequences per item
    if (!seq_off || !seq_len || 2 * (int64_t)nitems > 65535 || max_len <= 0 || total_rows <= 0)
        return mmdm_set_error(MMDM_ERR_ARG, "%s: bad sequence description nseq=%lld (<= 65535) max_len=%d total_rows=%d", who, 2 * (long long)nitems, max_len, total_rows);
    if ((!A && !planes) || Kp < MMDM_NF - 4 || lda < Kp) return mmdm_set_error(MMDM_ERR_ARG, "%s: bad operand Kp=%d lda=%d", who, Kp, lda);
    if (planes && plane_stride < (int64_t)total_rows * lda)
        return mmdm_set_error(MMDM_ERR_ARG, "%s: plane stride %lld < total_rows * lda = %lld", who, (long long)plane_stride, (long long)total_rows * lda);
    if (max_len - 1 > Tpad) return mmdm_set_error(MMDM_ERR_ARG, "%s: max_len=%d sequences need %d frames, the buffer holds %d", who, max_len, max_len - 1, Tpad);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(center_floor_kernel, dim3(nitems * 2), dim3(256), 0, st, motions, (long long)item_stride, row_stride, Tpad, 2, floor_ws);
    if (int rc = mmdm_check_launch("center_floor")) return rc;
    const dim3 grid((max_len + 7) / 8, nitems * 2), block(256);
    if (planes)
        hipLaunchKernelGGL(center_pack_kernel<true>, grid, block, 0, st, motions, (long long)item_stride, row_stride, Tpad, planes, (size_t)plane_stride, lda, Kp, seq_off,
                           seq_len, total_rows, floor_ws);
    else
        hipLaunchKernelGGL(center_pack_kernel<false>, grid, block, 0, st, motions, (long long)item_stride, row_stride, Tpad, static_cast<void*>(A), (size_t)0, lda, Kp, seq_off,
                           seq_len, total_rows, floor_ws);
    return mmdm_check_launch("center_pack");
}

extern "C" int mmdm_center_pack_f32(const float* motions, int64_t item_stride, int row_stride, int Tpad, int nitems, float* A, int lda, int Kp,
                                    const int* seq_off, const int* seq_len, int max_len, int total_rows, float* floor_ws, void* stream) {
    return center_pack("mmdm_center_pack_f32", motions, item_stride, row_stride, Tpad, nitems, A, nullptr, 0, lda, Kp, seq_off, seq_len, max_len, total_rows, floor_ws, stream);
}

extern "C" int mmdm_center_pack_split(const float* motions, int64_t item_stride, int row_stride, int Tpad, int nitems, void* planes, int lda, int64_t plane_stride, int Kp,
                                      const int* seq_off, const int* seq_len, int max_len, int total_rows, float* floor_ws, void* stream) {
    return center_pack("mmdm_center_pack_split", motions, item_stride, row_stride, Tpad, nitems, nullptr, planes, plane_stride, lda, Kp, seq_off, seq_len, max_len,
                       total_rows, floor_ws, stream);
}

// x2 == nullptr: the one-chain forms
int mmdm_pin_root(float* x, float* x2, const mmdm_opts_desc* od, const mmdm_rows& r, hipStream_t st) {
    if (r.fr) {
        const dim3 grid((r.fr->rows * 4 + 255) / 256);
        if (x2) hipLaunchKernelGGL(pin_root_rag_kernel<true>, grid, dim3(256), 0, st, x, x2, od, *r.fr);
        else hipLaunchKernelGGL(pin_root_rag_kernel<false>, grid, dim3(256), 0, st, x, x2, od, *r.fr);
        return mmdm_check_launch("pin_root_rag");
    }
    const dim3 grid((r.n * r.T * 4 + 255) / 256);
    if (x2) hipLaunchKernelGGL(pin_root_kernel<true>, grid, dim3(256), 0, st, x, x2, od, r.n, r.T);
    else hipLaunchKernelGGL(pin_root_kernel<false>, grid, dim3(256), 0, st, x, x2, od, r.n, r.T);
    return mmdm_check_launch("pin_root");
}

int mmdm_set_item_noise(const unsigned long long* seed_host, const int* row_host, int B, unsigned long long* item_seed, int* item_noise_row, hipStream_t st) {
    if (B <= 0 || B > MMDM_RAG_MAX_ITEMS || !seed_host) return mmdm_set_error(MMDM_ERR_ARG, "ragged batch: per-item seeds of %d items (1 .. %d)", B, MMDM_RAG_MAX_ITEMS);
    static_assert(MMDM_RAG_MAX_ITEMS <= 256, "one block of 256 threads writes the items");
    RagItemNoise v;
    for (int b = 0; b < MMDM_RAG_MAX_ITEMS; ++b) { v.seed[b] = b < B ? seed_host[b] : 0ull; v.row[b] = (b < B && row_host) ? row_host[b] : 0; }
    hipLaunchKernelGGL(set_item_noise_kernel, dim3(1), dim3(256), 0, st, v, B, item_seed, item_noise_row);
    return mmdm_check_launch("set_item_noise");
}

int mmdm_q_sample(float* x, float* x2, const float* init, float a, float b, size_t total, hipStream_t st) {
    const dim3 grid((unsigned)((total + 255) / 256));
    if (x2) hipLaunchKernelGGL(q_sample_kernel<true>, grid, dim3(256), 0, st, x, x2, init, a, b, total);
    else hipLaunchKernelGGL(q_sample_kernel<false>, grid, dim3(256), 0, st, x, x2, init, a, b, total);       // x2 == nullptr: one chain
    return mmdm_check_launch("q_sample");
}

int mmdm_set_opts_desc(mmdm_opts_desc* d, const mmdm_opts_desc& v, hipStream_t st) {
    hipLaunchKernelGGL(set_opts_kernel, dim3(1), dim3(1), 0, st, d, v);
    return mmdm_check_launch("set_opts");
}

extern "C" int mmdm_randn_f32(unsigned long long seed, int loop_pos, int B, int T, float* out, void* stream) {
    if (B == 0 || T == 0) return MMDM_OK;
    if (!out || B < 0 || T < 0 || loop_pos < 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_randn_f32: bad arguments");
    const size_t total = (size_t)B * T * NF2;
    hipLaunchKernelGGL(randn_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), seed, loop_pos, T, total, out);
    return mmdm_check_launch("randn");
}

extern "C" int mmdm_cfg_ddim_f32(const float* m, const float* coef, int S, const int* step_idx, float cfg_scale,
                                 float* x, float* pred_xstart, int B, int T, int C, void* stream) {
    if (B == 0 || T == 0) return MMDM_OK;
    if (!m || !coef || !step_idx || !x || S <= 0 || B < 0 || T < 0 || C <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_cfg_ddim_f32: bad arguments");
    const size_t total = (size_t)B * T * C;
    hipLaunchKernelGGL((cfg_ddim_kernel<false, 0>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       m, coef, S, step_idx, cfg_scale, x, pred_xstart, total);
    return mmdm_check_launch("cfg_ddim");
}

// The single-chain update with the loop's options (the stand-alone InterGen sampler): form as mmdm_xstart_ddim; r = the B items of the call (ragged: the group
// of r.fr->rows frame rows, whose uncond half of m follows at the group stride); C = 262 or 524.  Form 0 on uniform rows is mmdm_cfg_ddim_f32's launch.
int mmdm_cfg_ddim(int form, const float* m, const float* coef, const float* coef_eta, int S, const int* step_idx, const int* loop_pos, const mmdm_opts_desc* od,
                  float cfg_scale, float* x, float* pred_xstart, const mmdm_rows& r, int C, hipStream_t st) {
    if (form < 0 || form > 2) return mmdm_set_error(MMDM_ERR_ARG, "cfg_ddim: form %d", form);
    const size_t total = (r.fr ? (size_t)r.fr->rows : (size_t)r.n * r.T) * C;
    if (total == 0) return MMDM_OK;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const NoiseArgs na{coef_eta, od, loop_pos};
    const CfgRows cr{r.T, C, r.fr ? *r.fr : mmdm_rag{}};
    if (r.fr) {
        if (form == 0) hipLaunchKernelGGL((cfg_ddim_kernel<true, 0, CfgRows>), grid, block, 0, st, m, coef, S, step_idx, cfg_scale, x, pred_xstart, total, cr);
        else if (form == 1) hipLaunchKernelGGL((cfg_ddim_kernel<true, 1, CfgRows, NoiseArgs>), grid, block, 0, st, m, coef, S, step_idx, cfg_scale, x, pred_xstart, total, cr, na);
        else hipLaunchKernelGGL((cfg_ddim_kernel<true, 2, CfgRows, NoiseArgs>), grid, block, 0, st, m, coef, S, step_idx, cfg_scale, x, pred_xstart, total, cr, na);
        return mmdm_check_launch("cfg_ddim_rag");
    }
    if (form == 0) hipLaunchKernelGGL((cfg_ddim_kernel<false, 0>), grid, block, 0, st, m, coef, S, step_idx, cfg_scale, x, pred_xstart, total);
    else if (form == 1) hipLaunchKernelGGL((cfg_ddim_kernel<false, 1, CfgRows, NoiseArgs>), grid, block, 0, st, m, coef, S, step_idx, cfg_scale, x, pred_xstart, total, cr, na);
    else hipLaunchKernelGGL((cfg_ddim_kernel<false, 2, CfgRows, NoiseArgs>), grid, block, 0, st, m, coef, S, step_idx, cfg_scale, x, pred_xstart, total, cr, na);
    return mmdm_check_launch("cfg_ddim");
}

// the six forms of one update kernel (rows uniform / ragged x noise form 0 / 1 / 2); `...` = the kernel's own arguments up to per_batch_total
#define MMDM_LAUNCH_UPDATE_FORMS(KERNEL, ...)                                                                                                       \
    do {                                                                                                                                            \
        if (r.fr) {                                                                                                                                 \
            if (form == 0) hipLaunchKernelGGL((KERNEL<true, 0, CfgRows>), grid, block, 0, st, __VA_ARGS__, total, cr);                              \
            else if (form == 1) hipLaunchKernelGGL((KERNEL<true, 1, CfgRows, NoiseArgs>), grid, block, 0, st, __VA_ARGS__, total, cr, na);          \
            else hipLaunchKernelGGL((KERNEL<true, 2, CfgRows, NoiseArgs>), grid, block, 0, st, __VA_ARGS__, total, cr, na);                         \
        } else if (form == 0) hipLaunchKernelGGL((KERNEL<false, 0>), grid, block, 0, st, __VA_ARGS__, total);                                       \
        else if (form == 1) hipLaunchKernelGGL((KERNEL<false, 1, CfgRows, NoiseArgs>), grid, block, 0, st, __VA_ARGS__, total, cr, na);             \
        else hipLaunchKernelGGL((KERNEL<false, 2, CfgRows, NoiseArgs>), grid, block, 0, st, __VA_ARGS__, total, cr, na);                            \
    } while (0)

// The 4-way CFG update with the loop's options (single_only = 4, cfg_form = 1): form, r and C as mmdm_cfg_ddim; m holds the four CFG copies of the model
// output one after the other (ragged: at the group stride).  Form 0 on uniform rows is mmdm_cfg4_ddim_f32's launch.
int mmdm_cfg4_ddim(int form, const float* m, const float* coef, const float* coef_eta, int S, const int* step_idx, const int* loop_pos, const mmdm_opts_desc* od,
                   float s, float s_int, float s_ind, float* x, float* pred_xstart, const mmdm_rows& r, int C, hipStream_t st) {
    if (form < 0 || form > 2) return mmdm_set_error(MMDM_ERR_ARG, "cfg4_ddim: form %d", form);
    const size_t total = (r.fr ? (size_t)r.fr->rows : (size_t)r.n * r.T) * C;
    if (total == 0) return MMDM_OK;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const NoiseArgs na{coef_eta, od, loop_pos};
    const CfgRows cr{r.T, C, r.fr ? *r.fr : mmdm_rag{}};
    MMDM_LAUNCH_UPDATE_FORMS(cfg4_ddim_kernel, m, coef, S, step_idx, s, s_int, s_ind, x, pred_xstart);
    return mmdm_check_launch(r.fr ? "cfg4_ddim_rag" : "cfg4_ddim");
}

extern "C" int mmdm_cfg4_ddim_f32(const float* m, const float* coef, int S, const int* step_idx, float s, float s_int, float s_ind,
                                  float* x, float* pred_xstart, int B, int T, int C, void* stream) {
    if (B == 0 || T == 0) return MMDM_OK;
    if (!m || !coef || !step_idx || !x || S <= 0 || B < 0 || T < 0 || C <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_cfg4_ddim_f32: bad arguments");
    return mmdm_cfg4_ddim(0, m, coef, nullptr, S, step_idx, nullptr, nullptr, s, s_int, s_ind, x, pred_xstart, mmdm_rows{B, T}, C, static_cast<hipStream_t>(stream));
}

// The DualMDM update with the loop's options (single_only = 4, cfg_form = 2): m_ind / m_int hold the cond | uncond halves of the two models' outputs.
// Form 0 on uniform rows is mmdm_dual_ddim_f32's launch.
int mmdm_dual_ddim(int form, const float* m_ind, const float* m_int, const float* coef, const float* coef_eta, int S, const int* step_idx, const int* loop_pos,
                   const mmdm_opts_desc* od, const float* w_table, float s_ind, float s_int, float* x, float* pred_xstart, const mmdm_rows& r, int C, hipStream_t st) {
    if (form < 0 || form > 2) return mmdm_set_error(MMDM_ERR_ARG, "dual_ddim: form %d", form);
    const size_t total = (r.fr ? (size_t)r.fr->rows : (size_t)r.n * r.T) * C;
    if (total == 0) return MMDM_OK;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const NoiseArgs na{coef_eta, od, loop_pos};
    const CfgRows cr{r.T, C, r.fr ? *r.fr : mmdm_rag{}};
    MMDM_LAUNCH_UPDATE_FORMS(dual_ddim_kernel, m_ind, m_int, coef, S, step_idx, w_table, s_ind, s_int, x, pred_xstart);
    return mmdm_check_launch(r.fr ? "dual_ddim_rag" : "dual_ddim");
}
#undef MMDM_LAUNCH_UPDATE_FORMS

extern "C" int mmdm_dual_ddim_f32(const float* m_ind, const float* m_int, const float* coef, int S, const int* step_idx, const float* w_table,
                                  float s_ind, float s_int, float* x, float* pred_xstart, int B, int T, int C, void* stream) {
    if (B == 0 || T == 0) return MMDM_OK;
    if (!m_ind || !m_int || !coef || !step_idx || !w_table || !x || S <= 0 || B < 0 || T < 0 || C <= 0)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_dual_ddim_f32: bad arguments");
    return mmdm_dual_ddim(0, m_ind, m_int, coef, nullptr, S, step_idx, nullptr, nullptr, w_table, s_ind, s_int, x, pred_xstart, mmdm_rows{B, T}, C,
                          static_cast<hipStream_t>(stream));
}

// split != 0: dst receives [npers][2 planes][rows][ldp] fp16 (the A operand of mmdm_linear_split) instead of [npers][rows][ldp] fp32
int mmdm_repack_pose(const float* src, int ld_src, float* dst, int npers, int rows, int ldp, int split, hipStream_t st) {
    const size_t total = (size_t)npers * rows * ldp;
    if (total == 0) return MMDM_OK;
    if (split) hipLaunchKernelGGL(repack_pose_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, ld_src, reinterpret_cast<_Float16*>(dst), npers, rows, ldp);
    else hipLaunchKernelGGL(repack_pose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, ld_src, dst, npers, rows, ldp);
    return mmdm_check_launch("repack_pose");
}

extern "C" int mmdm_gather_rows_f32(const float* src, const int* idx, float* dst, int n, int D, void* stream) {
    if (n == 0) return MMDM_OK;
    if (!src || !idx || !dst || n < 0 || D <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_gather_rows_f32: bad arguments");
    return mmdm_gather_rows(src, idx, dst, n, D, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_ddim_reverse_f32(const float* x0, const float* coef, const float* rev, int S, const int* step_idx, float* x, int rows, int C,
                                    const int* row_item, void* stream) {
    if (rows == 0) return MMDM_OK;
    if (!x0 || !coef || !rev || !step_idx || !x || S <= 0 || rows < 0 || C <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_ddim_reverse_f32: bad arguments");
    const size_t total = (size_t)rows * C;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (row_item) hipLaunchKernelGGL((ddim_reverse_kernel<true>), grid, block, 0, st, x0, coef, rev, S, step_idx, x, total, row_item, C);
    else hipLaunchKernelGGL((ddim_reverse_kernel<false>), grid, block, 0, st, x0, coef, rev, S, step_idx, x, total, (const int*)nullptr, C);
    return mmdm_check_launch(row_item ? "ddim_reverse_rag" : "ddim_reverse");
}

int mmdm_step_dec(int* step_idx, int* loop_pos, hipStream_t st) {
    hipLaunchKernelGGL(step_dec_kernel, dim3(1), dim3(1), 0, st, step_idx, loop_pos);
    return mmdm_check_launch("step_dec");
}

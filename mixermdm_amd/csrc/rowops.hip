// Row-wise HBM-bound kernels of the denoising path (gfx950): AdaLN apply, conditioning-vector SiLU,
// time mean, Influence head.  One 64-lane wavefront per row, 16-byte loads, wave-shuffle reductions.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.h"

// This file is built TWICE (mixermdm_amd/build.py): rowops.o as it stands, and rowops_nopk.o with -DMMDM_ROWOPS_NOPK and without the packed-fp32
// VALU instructions -- the same kernels (inside `nopk::`, so that a kernel trace tells them apart).  Each build fills its own table of row operations
// (kernels.h mmdm_rowops: mmdm_rowops_tab / mmdm_rowops_tab_nopk); the handles of precision 1-3 take the second (mmdm.hip Ctx::ro): their row kernels run
// beside packed-W GEMMs, where dense packed-fp32 code was seen to compute other bits on gfx950 (build.py has the story; AdaLN itself was never seen to
// move -- tests/test_gpu_hazard.py holds that -- the second build removes the question instead of answering it).  The entry points of include/mmdm.h
// exist in the first build only.
#ifdef MMDM_ROWOPS_NOPK
#define RO(name) name##_nopk
#else
#define RO(name) name
#endif

namespace {
#ifdef MMDM_ROWOPS_NOPK
inline namespace nopk {
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifdef MMDM_ROWOPS_NOPK
// All-reduce over the wave WITHOUT the LDS (the second build only: the first keeps the bits of rounds 1-5).  __shfl_xor is a ds_bpermute: an LDS round
// trip per butterfly step, six in sequence per reduction, and AdaLN makes two (three with the fp8 row maximum) per row -- the fp8 form ran at 4.45 TB/s
// against the 5.7 of the two-reduction fp32 form although it moves fewer bytes.  Here: four DPP steps inside a 16-lane row (quad_perm 1032, quad_perm
// 2301, row_half_mirror, row_mirror: a VALU modifier, no LDS) and gfx950's v_permlane16_swap / v_permlane32_swap across the four rows (attn_f32.hip).
template <int CTRL>
__device__ __forceinline__ float dpp(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true)); }
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp<0xB1>(v); v += dpp<0x4E>(v); v += dpp<0x141>(v); v += dpp<0x140>(v);
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    a = a + b; b = a;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return a + b;
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp<0xB1>(v)); v = fmaxf(v, dpp<0x4E>(v)); v = fmaxf(v, dpp<0x141>(v)); v = fmaxf(v, dpp<0x140>(v));
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    a = fmaxf(a, b); b = a;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}
#else
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
#endif

// out = LN(h) * (1 + scale) + shift ; one wave per row; row cached in registers (D <= 64*4*MAXV).
// Reference: AdaLN.forward src/models/utils/layers.py:15-25 (LayerNorm eps 1e-6, biased variance, no affine).
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack_fp8x4(f32x4 v) {      // OCP e4m3, RNE, saturating at +-448 (as in gemm_bf16.hip)
    float c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = fminf(fmaxf(v[i], -448.f), 448.f);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], w, true);
    return (unsigned)w;
}

// OMODE: 0 fp32, 1 bf16, 2 the two fp16 planes of the fp32-split mode (kernels.h mmdm_split2, plane stride rows*D), 3 fp8 e4m3 with a per-row scale (row_scale[row] =
// max|y| / 448; the fp8 GEMM multiplies it back in its epilogue)
template <int MAXV, int OMODE>
__global__ __launch_bounds__(256, MAXV <= 4 ? 8 : 4) void adaln_kernel(const float* __restrict__ h, const float* __restrict__ ss, int ss_ld, int ss_rows,
                                                     void* __restrict__ outv, int rows, int T, int D, float* __restrict__ row_scale = nullptr,
                                                     const int* __restrict__ row_seq = nullptr) {     // ragged batch: sequence of every row (T unused)
    const int lane = threadIdx.x & 63;
    const int nv = D >> 2;                                   // float4 per row (D % 4 == 0 checked on host)
    // persistent: a fixed grid of wave slots walks the rows (one launch of ~2000 blocks instead of rows/4 short-lived ones)
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
    const float* hp = h + (size_t)row * D;
    f32x4 v[MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nv) v[i] = *reinterpret_cast<const f32x4*>(hp + 4 * c);
        s += v[i].x + v[i].y + v[i].z + v[i].w;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const f32x4 d = v[i] - mean;
            q += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-6f);
    const int sq = row_seq ? row_seq[row] : row / T;              // (wave-uniform)
    const float* sp = ss + (size_t)(sq % ss_rows) * ss_ld;
    if constexpr (OMODE == 3) {
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                const f32x4 sc = *reinterpret_cast<const f32x4*>(sp + 4 * c);
                const f32x4 sh = *reinterpret_cast<const f32x4*>(sp + D + 4 * c);
                v[i] = (v[i] - mean) * rstd * (1.0f + sc) + sh;
                amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[i][0]), fabsf(v[i][1])), fmaxf(fabsf(v[i][2]), fabsf(v[i][3]))));
            }
        }
        amax = wave_max(amax);
        const float scl = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f, inv = 1.0f / scl;
        if (lane == 0) row_scale[row] = scl;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(outv) + (size_t)row * D + 4 * c) = pack_fp8x4(v[i] * inv);
        }
        continue;
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const f32x4 sc = *reinterpret_cast<const f32x4*>(sp + 4 * c);
            const f32x4 sh = *reinterpret_cast<const f32x4*>(sp + D + 4 * c);
            const f32x4 y = (v[i] - mean) * rstd * (1.0f + sc) + sh;
            if (OMODE == 2) {
                mmdm_h4 oh, ol;
#pragma unroll
                for (int e = 0; e < 4; ++e) { const _Float16 t = mmdm_split_hi(y[e]); oh[e] = t; ol[e] = mmdm_split_lo(y[e], t); }
                _Float16* op = static_cast<_Float16*>(outv) + (size_t)row * D + 4 * c;
                const size_t plane = (size_t)rows * D;
                *reinterpret_cast<mmdm_h4*>(op) = oh;
                *reinterpret_cast<mmdm_h4*>(op + plane) = ol;
            } else if (OMODE == 1) {
                const bf16x4 o = {(__bf16)y[0], (__bf16)y[1], (__bf16)y[2], (__bf16)y[3]};
                *reinterpret_cast<bf16x4*>(static_cast<__bf16*>(outv) + (size_t)row * D + 4 * c) = o;
            } else {
                *reinterpret_cast<f32x4*>(static_cast<float*>(outv) + (size_t)row * D + 4 * c) = y;
            }
        }
    }
    }
}

// out = LN_{eps}(x) * gamma + beta (nn.LayerNorm with affine); one wave per row, row cached in registers, in place allowed.
// Reference: norm1 / norm2 of nn.TransformerEncoderLayer (src/models/mdm.py:252-264, src/models/mixermdm.py:246-259), clip_ln, ln_final.
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ out, int rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int nv = D >> 2;
    // persistent like adaln_kernel: the host caps the grid at 2048 blocks, so every wave slot walks rows with the grid's stride
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
    const float* xp = x + (size_t)row * D;
    f32x4 v[MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nv) v[i] = *reinterpret_cast<const f32x4*>(xp + 4 * c);
        s += v[i].x + v[i].y + v[i].z + v[i].w;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const f32x4 d = v[i] - mean;
            q += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
            const f32x4 b = *reinterpret_cast<const f32x4*>(beta + 4 * c);
            *reinterpret_cast<f32x4*>(out + (size_t)row * D + 4 * c) = (v[i] - mean) * rstd * g + b;
        }
    }
    }
}

// The same LayerNorm for the fp32-split post-norm encoder (MDMDenoiser, precision 2): a post-norm layer uses its normalised row twice -- as the
// residual of the next sub-layer (fp32) and as the next GEMM's A operand (the two fp16 planes h = fp16(y), l = fp16((y - h) * 2048): kernels.h) --
// so ONE pass reads the fp32 row, keeps it in registers (as adaln_kernel's OMODE 2 does) and writes the fp32 row and both planes.  The arithmetic
// of y is layernorm_kernel's, statement for statement: out is bitwise that kernel's, the planes are bitwise mmdm_split2 of it.
// planes: [2][rows][D] fp16, plane stride in elements.  In place (out == x) allowed.
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_split_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ out, _Float16* __restrict__ planes, size_t plane, int rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int nv = D >> 2;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
    const float* xp = x + (size_t)row * D;
    f32x4 v[MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nv) v[i] = *reinterpret_cast<const f32x4*>(xp + 4 * c);
        s += v[i].x + v[i].y + v[i].z + v[i].w;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const f32x4 d = v[i] - mean;
            q += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
            const f32x4 b = *reinterpret_cast<const f32x4*>(beta + 4 * c);
            const f32x4 y = (v[i] - mean) * rstd * g + b;
            *reinterpret_cast<f32x4*>(out + (size_t)row * D + 4 * c) = y;
            mmdm_h4 oh, ol;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const _Float16 t = mmdm_split_hi(y[e]); oh[e] = t; ol[e] = mmdm_split_lo(y[e], t); }
            _Float16* op = planes + (size_t)row * D + 4 * c;
            *reinterpret_cast<mmdm_h4*>(op) = oh;
            *reinterpret_cast<mmdm_h4*>(op + plane) = ol;
        }
    }
    }
}

// MDMDenoiser sequence assembly (src/models/mdm.py:279-294): dst [nseq, T+1, D];
//   dst[s, 0, :]   = (cond[s, :] + time_tab[*step, :]) + pe[0, :]         (the conditioning token; cond row stride ldc)
//   dst[s, 1+t, :] = src[s, t, :]                                          (pose embeddings, already + pe[1+t])
__global__ void mdm_pack_kernel(const float* __restrict__ src, const float* __restrict__ cond, int ldc, const float* __restrict__ time_tab,
                                const int* __restrict__ step_idx, const float* __restrict__ pe, float* __restrict__ dst, int nseq, int T, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nseq * (T + 1) * D) return;
    const int d = (int)(i % D);
    const size_t row = i / D;
    const int t = (int)(row % (T + 1));
    const size_t s = row / (T + 1);
    dst[i] = t == 0 ? (cond[s * ldc + d] + time_tab[(size_t)(*step_idx) * D + d]) + pe[d] : src[(s * T + (t - 1)) * D + d];
}

// dst[s, t, :] = src[s, 1+t, :]   (drop the conditioning token: mdm.py:296)
__global__ void mdm_unpack_kernel(const float* __restrict__ src, float* __restrict__ dst, int nseq, int T, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nseq * T * D) return;
    const int d = (int)(i % D);
    const size_t row = i / D;
    dst[i] = src[(row + row / T + 1) * D + d];
}

// The two passes on a RAGGED batch (kernels.h mmdm_rag): the frame rows of a group (`fr`: items back to back, stride fr.rows) and its token rows
// (`tk`: every item's conditioning token in front of its frames, stride tk.rows; tk.row_pos 0 = the token, k >= 1 = frame k - 1) are two row spaces.
//   dst[g, r, :] = 0                                                             padding token row (tk.row_item[r] < 0)
//                = (cond[(g % gpp) B + item, p D + :] + time_tab[*step, :]) + pe[0, :]     the token of `item`; p = g / gpp = the person of group g
//                = src[g, fr.item_off[item] + pos - 1, :]                        frame pos - 1 of `item`
// (same association order of the token's sum as mdm_pack_kernel: the bits of the uniform path)
__global__ void mdm_pack_rag_kernel(const float* __restrict__ src, const float* __restrict__ cond, int ldc, const float* __restrict__ time_tab,
                                    const int* __restrict__ step_idx, const float* __restrict__ pe, float* __restrict__ dst, int groups, int gpp, int D,
                                    mmdm_rag fr, mmdm_rag tk) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)groups * tk.rows * D) return;
    const int d = (int)(i % D);
    const size_t row = i / D;
    const int r = (int)(row % tk.rows), g = (int)(row / tk.rows);
    const int item = tk.row_item[r], pos = tk.row_pos[r];
    float y = 0.f;
    if (item >= 0) {
        if (pos == 0) y = (cond[((size_t)(g % gpp) * tk.B + item) * ldc + (size_t)(g / gpp) * D + d] + time_tab[(size_t)(*step_idx) * D + d]) + pe[d];
        else y = src[((size_t)g * fr.rows + fr.item_off[item] + (pos - 1)) * D + d];
    }
    dst[i] = y;
}

// mdm_pack_kernel / mdm_pack_rag_kernel for the fp32-split encoder (precision 2): the assembled rows are layer 0's residual (fp32, dst) AND the A operand
// of its QKV GEMM, so the same pass writes their two fp16 planes (planes [2][rows][D], plane stride in elements).  Four columns per thread (D % 4 == 0;
// every row of src / cond / time_tab / pe / dst starts on a 16-byte boundary): one 16-byte load, one 16-byte and two 8-byte stores.  The token's sum keeps
// mdm_pack_kernel's association order, so dst is bitwise that kernel's; padding token rows of the ragged form are zeros in dst and in both planes.
__device__ __forceinline__ void store_row4_split(float* __restrict__ dst, _Float16* __restrict__ planes, size_t plane, size_t i, const f32x4 y) {
    *reinterpret_cast<f32x4*>(dst + i) = y;
    mmdm_h4 oh, ol;
#pragma unroll
    for (int e = 0; e < 4; ++e) { const _Float16 t = mmdm_split_hi(y[e]); oh[e] = t; ol[e] = mmdm_split_lo(y[e], t); }
    *reinterpret_cast<mmdm_h4*>(planes + i) = oh;
    *reinterpret_cast<mmdm_h4*>(planes + plane + i) = ol;
}

__global__ void mdm_pack_split_kernel(const float* __restrict__ src, const float* __restrict__ cond, int ldc, const float* __restrict__ time_tab,
                                      const int* __restrict__ step_idx, const float* __restrict__ pe, float* __restrict__ dst, _Float16* __restrict__ planes,
                                      size_t plane, int nseq, int T, int D) {
    const int nv = D >> 2;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (size_t)nseq * (T + 1) * nv) return;
    const int d = 4 * (int)(j % nv);
    const size_t row = j / nv;
    const int t = (int)(row % (T + 1));
    const size_t s = row / (T + 1);
    f32x4 y;
    if (t == 0) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cond + s * ldc + d);
        const f32x4 tt = *reinterpret_cast<const f32x4*>(time_tab + (size_t)(*step_idx) * D + d);
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(pe + d);
        y = (c + tt) + p0;
    } else {
        y = *reinterpret_cast<const f32x4*>(src + (s * T + (t - 1)) * D + d);
    }
    store_row4_split(dst, planes, plane, row * D + d, y);
}

__global__ void mdm_pack_rag_split_kernel(const float* __restrict__ src, const float* __restrict__ cond, int ldc, const float* __restrict__ time_tab,
                                          const int* __restrict__ step_idx, const float* __restrict__ pe, float* __restrict__ dst, _Float16* __restrict__ planes,
                                          size_t plane, int groups, int gpp, int D, mmdm_rag fr, mmdm_rag tk) {
    const int nv = D >> 2;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (size_t)groups * tk.rows * nv) return;
    const int d = 4 * (int)(j % nv);
    const size_t row = j / nv;
    const int r = (int)(row % tk.rows), g = (int)(row / tk.rows);
    const int item = tk.row_item[r], pos = tk.row_pos[r];
    f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f};
    if (item >= 0) {
        if (pos == 0) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(cond + ((size_t)(g % gpp) * tk.B + item) * ldc + (size_t)(g / gpp) * D + d);
            const f32x4 tt = *reinterpret_cast<const f32x4*>(time_tab + (size_t)(*step_idx) * D + d);
            const f32x4 p0 = *reinterpret_cast<const f32x4*>(pe + d);
            y = (c + tt) + p0;
        } else {
            y = *reinterpret_cast<const f32x4*>(src + ((size_t)g * fr.rows + fr.item_off[item] + (pos - 1)) * D + d);
        }
    }
    store_row4_split(dst, planes, plane, row * D + d, y);
}

// dst[g, r, :] = src[g, tk.item_off[item] + 1 + pos, :] for frame row r = (item, pos) of a group; padding frame rows are written as zeros
__global__ void mdm_unpack_rag_kernel(const float* __restrict__ src, float* __restrict__ dst, int groups, int D, mmdm_rag fr, mmdm_rag tk) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)groups * fr.rows * D) return;
    const int d = (int)(i % D);
    const size_t row = i / D;
    const int r = (int)(row % fr.rows), g = (int)(row / fr.rows);
    const int item = fr.row_item[r];
    dst[i] = item < 0 ? 0.f : src[((size_t)g * tk.rows + tk.item_off[item] + 1 + fr.row_pos[r]) * D + d];
}

// out[b, l, :] = table[tokens[b, l], :] + pos[l, :]   (CLIP token + positional embedding: src/models/mixermdm.py:298-299)
__global__ void token_embed_kernel(const float* __restrict__ table, const int* __restrict__ tokens, const float* __restrict__ pos,
                                   float* __restrict__ out, int n, int L, int D, int vocab) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * L * D) return;
    const int d = (int)(i % D);
    const size_t row = i / D;
    int tok = tokens[row];
    tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
    out[i] = table[(size_t)tok * D + d] + pos[(row % L) * D + d];
}

__global__ void cond_silu_kernel(const float* __restrict__ time_tab, const int* __restrict__ step_idx, const float* __restrict__ txt,
                                 float* __restrict__ out, int rows, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * D) return;
    const int d = (int)(i % D);
    const float e = time_tab[(size_t)(*step_idx) * D + d] + txt[i];
    out[i] = e / (1.0f + expf(-e));
}

// the same rows as the two fp16 operand planes of the fp32-split GEMM (out[i], out[plane + i]): cond_vectors of the low-precision handles
__global__ void cond_silu_planes_kernel(const float* __restrict__ time_tab, const int* __restrict__ step_idx, const float* __restrict__ txt,
                                        _Float16* __restrict__ out, size_t plane, int rows, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * D) return;
    const int d = (int)(i % D);
    const float e = time_tab[(size_t)(*step_idx) * D + d] + txt[i];
    _Float16 h, l;
    mmdm_split2(e / (1.0f + expf(-e)), h, l);
    out[i] = h;
    out[plane + i] = l;
}

__global__ void mean_time_kernel(const float* __restrict__ h, float* __restrict__ out, int T, int D) {
    const int seq = blockIdx.y;
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const float* p = h + (size_t)seq * T * D + d;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += p[(size_t)t * D];
    out[(size_t)seq * D + d] = s / (float)T;
}

// ragged batch: sequence s = rows [seq_off[s], seq_off[s] + seq_len[s]) of h (same summation order as mean_time_kernel: bit-identical per sequence)
__global__ void mean_time_rag_kernel(const float* __restrict__ h, float* __restrict__ out, const int* __restrict__ seq_off, const int* __restrict__ seq_len, int D) {
    const int seq = blockIdx.y;
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const int T = seq_len[seq];
    const float* p = h + (size_t)seq_off[seq] * D + d;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += p[(size_t)t * D];
    out[(size_t)seq * D + d] = s / (float)T;
}

// w[row, o] = sigmoid(h[row,:] . Wout[o,:] + b[o]); one wave per row, nw <= 23 outputs.
// Reference: Influence.forward tail src/models/utils/influence.py:124-125.
__global__ __launch_bounds__(256) void influence_head_kernel(const float* __restrict__ h, const float* __restrict__ W, const float* __restrict__ b,
                                                              float* __restrict__ w, int rows, int D, int nw) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* hp = h + (size_t)row * D;
    for (int o = 0; o < nw; ++o) {
        const float* wp = W + (size_t)o * D;
        float s = 0.f;
        for (int c = lane; c < D; c += 64) s += hp[c] * wp[c];
        s = wave_sum(s);
        if (lane == 0) {
            const float z = s + b[o];
            w[(size_t)row * nw + o] = 1.0f / (1.0f + expf(-z));
        }
    }
}

// scipy.ndimage.gaussian_filter1d(x, sigma, axis=time, mode="nearest") on [n, T, C]: correlate with a symmetric kernel of
// radius r, indices clamped to [0, T-1]; weights and accumulation in double (scipy's correlate1d accumulates in double).
__global__ void gauss1d_kernel(const float* __restrict__ x, float* __restrict__ out, const double* __restrict__ w, int radius, int n, int T, int C) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * T * C) return;
    const int c = (int)(idx % C);
    const int t = (int)((idx / C) % T);
    const size_t b = idx / ((size_t)C * T);
    const float* xb = x + b * T * C + c;
    double acc = 0.0;
    for (int k = -radius; k <= radius; ++k) {
        int tt = t + k;
        tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
        acc += w[k + radius] * (double)xb[(size_t)tt * C];
    }
    out[idx] = (float)acc;
}

// InterCLIP's MotionEncoder (src/evaluation/models.py:57-66) on a RAGGED batch: item s is a token sequence of seq_len[s] rows -- the query token, then its
// first seq_len[s] - 1 frames -- at rows [seq_off[s], seq_off[s] + seq_len[s]).  One wave per row: blockIdx.y = the item, wave blockIdx.x * 4 + w = the
// position p inside it (the grid is sized by the longest item; waves past an item's end leave).
// A[row, q * 258 + j] = motions[s, p - 1, q * 262 + j] for j < 258 (x.reshape(B, T, 2, -1)[..., :-4]); columns [npers * 258, Kp) and the token row are zeros.
// Frames at and beyond seq_len[s] - 1 are never read.  A plain 4-byte loop: person 1 starts 1048 bytes into a motion row and 1032 bytes into an A row, so the
// two sides share no 16-byte phase; consecutive lanes still read and write consecutive words.
template <bool SPLIT>
__global__ __launch_bounds__(256) void motion_pack_kernel(const float* __restrict__ motions, long long item_stride, int row_stride, int Tpad, int npers,
                                                           void* __restrict__ Av, size_t plane, int lda, int Kp, const int* __restrict__ seq_off,
                                                           const int* __restrict__ seq_len, int total_rows) {
    const int s = blockIdx.y, p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= seq_len[s] || p > Tpad) return;                     // (wave-uniform)
    const long long row = (long long)seq_off[s] + p;
    if (row < 0 || row >= total_rows) return;
    const int K = npers * (MMDM_NF - 4);
    const float* mp = motions + (size_t)s * item_stride + (size_t)(p > 0 ? p - 1 : 0) * row_stride;
    for (int c = lane; c < Kp; c += 64) {
        float v = 0.f;
        if (p > 0 && c < K) {
            const int q = c / (MMDM_NF - 4);
            v = mp[q * MMDM_NF + (c - q * (MMDM_NF - 4))];
        }
        if constexpr (SPLIT) {      // the operand of the fp32-split embedding GEMM: the same element as its two fp16 planes (a zero is +0 in both)
            _Float16* ap = static_cast<_Float16*>(Av) + (size_t)row * lda;
            _Float16 hi, lo;
            mmdm_split2(v, hi, lo);
            ap[c] = hi;
            ap[plane + c] = lo;
        } else {
            static_cast<float*>(Av)[(size_t)row * lda + c] = v;
        }
    }
}

// In place on the embedding GEMM's output h [total_rows, D] (same row walk): the token row becomes query + pe[0], frame row p gets += pe[p]
// (PositionalEncoding after the token is prepended: src/models/utils/utils.py:37-39).  D % 4 == 0, 16-byte rows.
// SPLIT: the rows are layer 0's residual AND the operand of its QKV GEMM in the fp32-split mode, so the same pass writes their two fp16 planes
// (planes [2][total_rows][D], plane stride in elements) -- the role mdm_pack_split_kernel plays for MDM; h is bitwise the plain form's.
template <bool SPLIT>
__global__ __launch_bounds__(256) void motion_tokens_kernel(float* __restrict__ h, _Float16* __restrict__ planes, size_t plane, const float* __restrict__ query,
                                                             const float* __restrict__ pe, int D, const int* __restrict__ seq_off,
                                                             const int* __restrict__ seq_len, int total_rows) {
    const int s = blockIdx.y, p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= seq_len[s]) return;                                 // (wave-uniform)
    const long long row = (long long)seq_off[s] + p;
    if (row < 0 || row >= total_rows) return;
    float* hp = h + (size_t)row * D;
    const float* pp = pe + (size_t)p * D;
    for (int c = lane; c < (D >> 2); c += 64) {
        const f32x4 e = *reinterpret_cast<const f32x4*>(pp + 4 * c);
        const f32x4 a = p == 0 ? *reinterpret_cast<const f32x4*>(query + 4 * c) : *reinterpret_cast<const f32x4*>(hp + 4 * c);
        if constexpr (SPLIT) store_row4_split(h, planes, plane, (size_t)row * D + 4 * c, a + e);
        else *reinterpret_cast<f32x4*>(hp + 4 * c) = a + e;
    }
}

// out[row] = x[row] / ||x[row]||_2 * scale[0]  (InterCLIP.encode_motion / encode_text: src/evaluation/models.py:152, 178).  One wave per row, the row in
// registers; the sum of squares is a lane's own columns in ascending order, then the wave reduction: a row's bits do not depend on `rows`.  In place allowed.
template <int MAXV>
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, const float* __restrict__ scale, float* __restrict__ out, int rows, int D) {
    const int lane = threadIdx.x & 63;
    const int nv = D >> 2;
    const float sc = scale[0];
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
        const float* xp = x + (size_t)row * D;
        f32x4 v[MAXV];
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < nv) v[i] = *reinterpret_cast<const f32x4*>(xp + 4 * c);
            q += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
        }
        const float nrm = sqrtf(wave_sum(q));
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) *reinterpret_cast<f32x4*>(out + (size_t)row * D + 4 * c) = v[i] / nrm * sc;
        }
    }
}

#ifdef MMDM_ROWOPS_NOPK
}  // namespace nopk
#endif
}  // namespace

// ------------------------------------------------------------------------------------------------------
// Host side.  The launchers of this build's row operations have internal linkage: the rest of the library reaches them through the build's table
// (kernels.h mmdm_rowops; defined below them), the stateless entry points of include/mmdm.h -- first build only -- forward to them.
// ------------------------------------------------------------------------------------------------------
// row_seq != nullptr: ragged batch -- `rows_rag` rows in all, row r belongs to sequence row_seq[r] (device array); nseq / T are then unused
static int adaln_any(const float* h, const float* ss, int ss_ld, int ss_rows, void* out, int out_bf16, float* row_scale, int nseq, int T, int D, void* stream,
                     const int* row_seq, int rows_rag) {
    if (row_seq) { nseq = 1; T = rows_rag; }
    if (nseq == 0 || T == 0) return MMDM_OK;
    if (!h || !ss || !out || nseq < 0 || T < 0 || D <= 0 || ss_rows <= 0 || ss_ld < 2 * D)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_adaln_f32: bad arguments nseq=%d T=%d D=%d ss_ld=%d ss_rows=%d", nseq, T, D, ss_ld, ss_rows);
    if ((D & 3) || (ss_ld & 3) || ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(ss) | reinterpret_cast<uintptr_t>(out)) & 15))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_adaln_f32: D and ss_ld must be multiples of 4 and pointers 16-byte aligned");
    if (D > 64 * 4 * 8) return mmdm_set_error(MMDM_ERR_UNSUPPORTED, "mmdm_adaln_f32: D=%d > 2048", D);
    const int rows = nseq * T;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid(min((rows + 3) / 4, 2048)), block(256);          // 256 CUs x 8 resident blocks
#define ADALN_LAUNCH(V)                                                                                                   \
    do {                                                                                                                  \
        if (out_bf16 == 3) hipLaunchKernelGGL((adaln_kernel<V, 3>), grid, block, 0, st, h, ss, ss_ld, ss_rows, out, rows, T, D, row_scale, row_seq);       \
        else if (out_bf16 == 2) hipLaunchKernelGGL((adaln_kernel<V, 2>), grid, block, 0, st, h, ss, ss_ld, ss_rows, out, rows, T, D, (float*)nullptr, row_seq);       \
        else if (out_bf16) hipLaunchKernelGGL((adaln_kernel<V, 1>), grid, block, 0, st, h, ss, ss_ld, ss_rows, out, rows, T, D, (float*)nullptr, row_seq);       \
        else hipLaunchKernelGGL((adaln_kernel<V, 0>), grid, block, 0, st, h, ss, ss_ld, ss_rows, out, rows, T, D, (float*)nullptr, row_seq);                     \
    } while (0)
    if (D <= 256) ADALN_LAUNCH(1);
    else if (D <= 512) ADALN_LAUNCH(2);
    else if (D <= 1024) ADALN_LAUNCH(4);
    else ADALN_LAUNCH(8);
#undef ADALN_LAUNCH
    return mmdm_check_launch("adaln");
}

static int layernorm(const float* x, const float* gamma, const float* beta, float* out, int rows, int D, float eps, void* stream) {
    if (rows == 0) return MMDM_OK;
    if (!x || !gamma || !beta || !out || rows < 0 || D <= 0 || !(eps > 0.f)) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_layernorm_f32: bad arguments rows=%d D=%d", rows, D);
    if ((D & 3) || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) | reinterpret_cast<uintptr_t>(out)) & 15))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_layernorm_f32: D must be a multiple of 4 and pointers 16-byte aligned");
    if (D > 64 * 4 * 8) return mmdm_set_error(MMDM_ERR_UNSUPPORTED, "mmdm_layernorm_f32: D=%d > 2048", D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid(min((rows + 3) / 4, 2048)), block(256);          // 256 CUs x 8 resident blocks
    if (D <= 256) hipLaunchKernelGGL((layernorm_kernel<1>), grid, block, 0, st, x, gamma, beta, out, rows, D, eps);
    else if (D <= 512) hipLaunchKernelGGL((layernorm_kernel<2>), grid, block, 0, st, x, gamma, beta, out, rows, D, eps);
    else if (D <= 1024) hipLaunchKernelGGL((layernorm_kernel<4>), grid, block, 0, st, x, gamma, beta, out, rows, D, eps);
    else hipLaunchKernelGGL((layernorm_kernel<8>), grid, block, 0, st, x, gamma, beta, out, rows, D, eps);
    return mmdm_check_launch("layernorm");
}

// LayerNorm into the fp32 row AND its two fp16 planes (layernorm_split_kernel); the argument rules of layernorm, plus 16-byte aligned planes
static int layernorm_planes(const float* x, const float* gamma, const float* beta, float* out, void* planes, int64_t plane_stride, int rows, int D, float eps,
                            hipStream_t st) {
    if (rows == 0) return MMDM_OK;
    if (!x || !gamma || !beta || !out || !planes || rows < 0 || D <= 0 || !(eps > 0.f))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_layernorm_split: bad arguments rows=%d D=%d", rows, D);
    if ((D & 3) || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) | reinterpret_cast<uintptr_t>(out)) & 15))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_layernorm_split: D must be a multiple of 4 and pointers 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(planes) & 15) || (plane_stride & 7) || plane_stride < (int64_t)rows * D)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_layernorm_split: the planes must be 16-byte aligned, with a plane stride >= rows * D that is a multiple of 8 (stride=%lld)",
                              (long long)plane_stride);
    if (D > 64 * 4 * 8) return mmdm_set_error(MMDM_ERR_UNSUPPORTED, "mmdm_layernorm_split: D=%d > 2048", D);
    dim3 grid(min((rows + 3) / 4, 2048)), block(256);          // persistent wave slots, as layernorm
    _Float16* pl = static_cast<_Float16*>(planes);
    const size_t ps = (size_t)plane_stride;
    if (D <= 256) hipLaunchKernelGGL((layernorm_split_kernel<1>), grid, block, 0, st, x, gamma, beta, out, pl, ps, rows, D, eps);
    else if (D <= 512) hipLaunchKernelGGL((layernorm_split_kernel<2>), grid, block, 0, st, x, gamma, beta, out, pl, ps, rows, D, eps);
    else if (D <= 1024) hipLaunchKernelGGL((layernorm_split_kernel<4>), grid, block, 0, st, x, gamma, beta, out, pl, ps, rows, D, eps);
    else hipLaunchKernelGGL((layernorm_split_kernel<8>), grid, block, 0, st, x, gamma, beta, out, pl, ps, rows, D, eps);
    return mmdm_check_launch("layernorm_split");
}

// The sequence assembly: uniform r.n sequences of r.T frames -> T + 1 token rows each; ragged r.n / fr->B frame groups `fr` -> token groups `tk`, `gpp` groups per
// person (the CFG halves).  planes != null (precision 2): the rows' two fp16 planes as a second output (mdm_pack_split_kernel / mdm_pack_rag_split_kernel)
static int mdm_pack(const float* src, const float* cond, int ldc, const float* time_tab, const int* step_idx, const float* pe, float* dst, void* planes,
                    int64_t plane_stride, const mmdm_rows& r, int gpp, int D, hipStream_t st) {
    if (r.fr && !r.tk) return mmdm_set_error(MMDM_ERR_STATE, "mdm_pack_rag: no token rows");
    const int groups = r.fr ? r.n / r.fr->B : 0;
    const size_t n = (r.fr ? (size_t)groups * r.tk->rows : (size_t)r.n * (r.T + 1)) * (planes ? D >> 2 : D);      // threads: one per element, or per four with planes
    if (n == 0) return MMDM_OK;
    if (planes && ((D & 3) || (ldc & 3) || (plane_stride & 7) || ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(cond) | reinterpret_cast<uintptr_t>(time_tab) |
                                                                  reinterpret_cast<uintptr_t>(pe) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(planes)) & 15)))
        return mmdm_set_error(MMDM_ERR_ARG, "mdm_pack%s (split): D and the cond stride must be multiples of 4 and every row 16-byte aligned (D=%d ldc=%d)", r.fr ? "_rag" : "", D, ldc);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    _Float16* pl = static_cast<_Float16*>(planes);
    if (r.fr && planes)
        hipLaunchKernelGGL(mdm_pack_rag_split_kernel, grid, block, 0, st, src, cond, ldc, time_tab, step_idx, pe, dst, pl, (size_t)plane_stride, groups, gpp, D, *r.fr, *r.tk);
    else if (r.fr) hipLaunchKernelGGL(mdm_pack_rag_kernel, grid, block, 0, st, src, cond, ldc, time_tab, step_idx, pe, dst, groups, gpp, D, *r.fr, *r.tk);
    else if (planes) hipLaunchKernelGGL(mdm_pack_split_kernel, grid, block, 0, st, src, cond, ldc, time_tab, step_idx, pe, dst, pl, (size_t)plane_stride, r.n, r.T, D);
    else hipLaunchKernelGGL(mdm_pack_kernel, grid, block, 0, st, src, cond, ldc, time_tab, step_idx, pe, dst, r.n, r.T, D);
    return mmdm_check_launch(r.fr ? "mdm_pack_rag" : "mdm_pack");
}

static int mdm_unpack(const float* src, float* dst, const mmdm_rows& r, int D, hipStream_t st) {
    if (r.fr && !r.tk) return mmdm_set_error(MMDM_ERR_STATE, "mdm_unpack_rag: no token rows");
    const int groups = r.fr ? r.n / r.fr->B : 0;
    const size_t n = (r.fr ? (size_t)groups * r.fr->rows : (size_t)r.n * r.T) * D;
    if (n == 0) return MMDM_OK;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (r.fr) hipLaunchKernelGGL(mdm_unpack_rag_kernel, grid, block, 0, st, src, dst, groups, D, *r.fr, *r.tk);
    else hipLaunchKernelGGL(mdm_unpack_kernel, grid, block, 0, st, src, dst, r.n, r.T, D);
    return mmdm_check_launch(r.fr ? "mdm_unpack_rag" : "mdm_unpack");
}

static int cond_silu(const float* time_tab, const int* step_idx, const float* txt, float* out, int rows, int D, void* stream) {
    if (rows == 0) return MMDM_OK;
    if (!time_tab || !step_idx || !txt || !out || rows < 0 || D <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_cond_silu_f32: bad arguments");
    const size_t n = (size_t)rows * D;
    hipLaunchKernelGGL(cond_silu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), time_tab, step_idx, txt, out, rows, D);
    return mmdm_check_launch("cond_silu");
}

static int cond_silu_planes(const float* time_tab, const int* step_idx, const float* txt, _Float16* out, size_t plane, int rows, int D, hipStream_t st) {
    if (rows == 0) return MMDM_OK;
    const size_t n = (size_t)rows * D;
    hipLaunchKernelGGL(cond_silu_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, time_tab, step_idx, txt, out, plane, rows, D);
    return mmdm_check_launch("cond_silu_planes");
}

// ragged (r.seq_off): sequence s = rows [seq_off[s], seq_off[s] + seq_len[s]) of h
static int mean_time(const float* h, float* out, const mmdm_rows& r, int D, hipStream_t st) {
    if (r.n == 0) return MMDM_OK;
    if (r.seq_off) {
        hipLaunchKernelGGL(mean_time_rag_kernel, dim3((D + 255) / 256, r.n), dim3(256), 0, st, h, out, r.seq_off, r.seq_len, D);
        return mmdm_check_launch("mean_time_rag");
    }
    if (!h || !out || r.n < 0 || r.T <= 0 || D <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_mean_time_f32: bad arguments");
    hipLaunchKernelGGL(mean_time_kernel, dim3((D + 255) / 256, r.n), dim3(256), 0, st, h, out, r.T, D);
    return mmdm_check_launch("mean_time");
}

// the ragged token sequences of the two motion-encoder passes: device arrays, a grid of (positions of the longest sequence / 4, sequences)
static int motion_seq_check(const char* who, int nseq, const int* seq_off, const int* seq_len, int max_len, int total_rows) {
    if (!seq_off || !seq_len || nseq < 0 || nseq > 65535 || max_len <= 0 || total_rows <= 0)
        return mmdm_set_error(MMDM_ERR_ARG, "%s: bad sequence description nseq=%d (<= 65535) max_len=%d total_rows=%d", who, nseq, max_len, total_rows);
    return MMDM_OK;
}

// A (fp32 rows) or planes (the same rows as the two fp16 planes of the fp32-split GEMM's A operand, [2][total_rows][lda], plane stride in elements): exactly one
static int motion_pack(const float* motions, int64_t item_stride, int row_stride, int Tpad, int npers, float* A, void* planes, int64_t plane_stride, int lda, int Kp,
                       int nseq, const int* seq_off, const int* seq_len, int max_len, int total_rows, hipStream_t st) {
    if (nseq == 0) return MMDM_OK;
    if (int rc = motion_seq_check("mmdm_rowop_motion_pack", nseq, seq_off, seq_len, max_len, total_rows)) return rc;
    if (!motions || (A != nullptr) == (planes != nullptr) || npers < 1 || npers > 2 || Tpad < 0 || row_stride < npers * MMDM_NF || item_stride < (int64_t)Tpad * row_stride ||
        Kp < npers * (MMDM_NF - 4) || lda < Kp)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_pack: bad arguments npers=%d Tpad=%d row stride=%d item stride=%lld Kp=%d lda=%d", npers, Tpad, row_stride,
                              (long long)item_stride, Kp, lda);
    if (planes && plane_stride < (int64_t)total_rows * lda)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_pack_split: plane stride %lld < total_rows * lda = %lld", (long long)plane_stride, (long long)total_rows * lda);
    if (max_len - 1 > Tpad) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_pack: max_len=%d sequences need %d frames, the buffer holds %d", max_len, max_len - 1, Tpad);
    const dim3 grid((max_len + 3) / 4, nseq), block(256);
    if (planes)
        hipLaunchKernelGGL(motion_pack_kernel<true>, grid, block, 0, st, motions, (long long)item_stride, row_stride, Tpad, npers, planes, (size_t)plane_stride, lda, Kp,
                           seq_off, seq_len, total_rows);
    else
        hipLaunchKernelGGL(motion_pack_kernel<false>, grid, block, 0, st, motions, (long long)item_stride, row_stride, Tpad, npers, static_cast<void*>(A), (size_t)0, lda, Kp,
                           seq_off, seq_len, total_rows);
    return mmdm_check_launch("motion_pack");
}

// planes != null: the rows' two fp16 planes [2][total_rows][D] as a second output (plane stride in elements)
static int motion_tokens(float* h, void* planes, int64_t plane_stride, const float* query, const float* pe, int pe_rows, int D, int nseq, const int* seq_off,
                         const int* seq_len, int max_len, int total_rows, hipStream_t st) {
    if (nseq == 0) return MMDM_OK;
    if (int rc = motion_seq_check("mmdm_rowop_motion_tokens", nseq, seq_off, seq_len, max_len, total_rows)) return rc;
    if (!h || !query || !pe || D <= 0 || pe_rows <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_tokens: bad arguments D=%d pe_rows=%d", D, pe_rows);
    if ((D & 3) || ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(pe)) & 15))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_tokens: D must be a multiple of 4 and pointers 16-byte aligned");
    if (planes && (plane_stride < (int64_t)total_rows * D || (plane_stride & 3) || (reinterpret_cast<uintptr_t>(planes) & 7)))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_tokens_split: planes must be 8-byte aligned with a stride %% 4 == 0 of at least total_rows * D (stride=%lld)",
                              (long long)plane_stride);
    // the grid's positions are rounded up to whole blocks of 4 waves: every position a wave can take has a pe row
    if ((max_len + 3) / 4 * 4 > pe_rows) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_tokens: max_len=%d needs more than the %d pe rows", max_len, pe_rows);
    const dim3 grid((max_len + 3) / 4, nseq), block(256);
    if (planes)
        hipLaunchKernelGGL(motion_tokens_kernel<true>, grid, block, 0, st, h, static_cast<_Float16*>(planes), (size_t)plane_stride, query, pe, D, seq_off, seq_len, total_rows);
    else hipLaunchKernelGGL(motion_tokens_kernel<false>, grid, block, 0, st, h, static_cast<_Float16*>(nullptr), (size_t)0, query, pe, D, seq_off, seq_len, total_rows);
    return mmdm_check_launch("motion_tokens");
}

static int l2_normalize(const float* x, const float* scale, float* out, int rows, int D, hipStream_t st) {
    if (rows == 0) return MMDM_OK;
    if (!x || !scale || !out || rows < 0 || D <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_l2_normalize_rows_f32: bad arguments rows=%d D=%d", rows, D);
    if ((D & 3) || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) || (reinterpret_cast<uintptr_t>(scale) & 3))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_l2_normalize_rows_f32: D must be a multiple of 4 and x / out 16-byte aligned");
    if (D > 64 * 4 * 8) return mmdm_set_error(MMDM_ERR_UNSUPPORTED, "mmdm_l2_normalize_rows_f32: D=%d > 2048", D);
    dim3 grid(min((rows + 3) / 4, 2048)), block(256);          // persistent wave slots, as layernorm
    if (D <= 256) hipLaunchKernelGGL((l2_normalize_kernel<1>), grid, block, 0, st, x, scale, out, rows, D);
    else if (D <= 512) hipLaunchKernelGGL((l2_normalize_kernel<2>), grid, block, 0, st, x, scale, out, rows, D);
    else if (D <= 1024) hipLaunchKernelGGL((l2_normalize_kernel<4>), grid, block, 0, st, x, scale, out, rows, D);
    else hipLaunchKernelGGL((l2_normalize_kernel<8>), grid, block, 0, st, x, scale, out, rows, D);
    return mmdm_check_launch("l2_normalize");
}

static int token_embed(const float* table, int vocab, const int* tokens, const float* pos, float* out, int n, int L, int D, hipStream_t st) {
    if (n == 0 || L == 0) return MMDM_OK;
    if (!table || !tokens || !pos || !out || n < 0 || L < 0 || D <= 0 || vocab <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_token_embed_f32: bad arguments");
    const size_t total = (size_t)n * L * D;
    hipLaunchKernelGGL(token_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, table, tokens, pos, out, n, L, D, vocab);
    return mmdm_check_launch("token_embed");
}

// (host pass only: the device pass would emit a constant of external linkage too, and has no such functions to point at)
#ifndef __HIP_DEVICE_COMPILE__
const mmdm_rowops RO(mmdm_rowops_tab) = {adaln_any, layernorm,  layernorm_planes, cond_silu,     cond_silu_planes, mean_time,
                                         mdm_pack,  mdm_unpack, motion_pack,      motion_tokens, l2_normalize,     token_embed};
#endif

#ifndef MMDM_ROWOPS_NOPK
extern "C" int mmdm_gaussian_filter1d_f32(const float* x, float* out, const double* weights, int radius, int n, int T, int C, void* stream) {
    if (n == 0 || T == 0 || C == 0) return MMDM_OK;
    if (!x || !out || !weights || radius < 0 || n < 0 || T < 0 || C < 0 || x == out)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_gaussian_filter1d_f32: bad arguments (in-place is not supported)");
    const size_t total = (size_t)n * T * C;
    hipLaunchKernelGGL(gauss1d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, weights, radius, n, T, C);
    return mmdm_check_launch("gauss1d");
}

extern "C" int mmdm_adaln_f32(const float* h, const float* ss, int ss_ld, int ss_rows, float* out, int nseq, int T, int D, void* stream) {
    return mmdm_adaln_ex(h, ss, ss_ld, ss_rows, out, 0, nseq, T, D, stream);
}

extern "C" int mmdm_adaln_ex(const float* h, const float* ss, int ss_ld, int ss_rows, void* out, int out_bf16, int nseq, int T, int D, void* stream) {
    if (out_bf16 < 0 || out_bf16 > 2) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_adaln_ex: output mode must be 0 (fp32), 1 (bf16) or 2 (the two fp16 planes of the fp32-split mode)");
    return adaln_any(h, ss, ss_ld, ss_rows, out, out_bf16, nullptr, nseq, T, D, stream, nullptr, 0);
}

extern "C" int mmdm_adaln_fp8(const float* h, const float* ss, int ss_ld, int ss_rows, void* out, float* row_scale, int nseq, int T, int D, void* stream) {
    if (!row_scale) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_adaln_fp8: null row_scale");
    return adaln_any(h, ss, ss_ld, ss_rows, out, 3, row_scale, nseq, T, D, stream, nullptr, 0);
}

extern "C" int mmdm_layernorm_f32(const float* x, const float* gamma, const float* beta, float* out, int rows, int D, float eps, void* stream) {
    return layernorm(x, gamma, beta, out, rows, D, eps, stream);
}

extern "C" int mmdm_cond_silu_f32(const float* time_tab, const int* step_idx, const float* txt, float* out, int rows, int D, void* stream) {
    return cond_silu(time_tab, step_idx, txt, out, rows, D, stream);
}

extern "C" int mmdm_mean_time_f32(const float* h, float* out, int nseq, int T, int D, void* stream) {
    return mean_time(h, out, mmdm_rows{nseq, T}, D, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_token_embed_f32(const float* table, int vocab, const int* tokens, const float* pos, float* out, int n, int L, int D, void* stream) {
    return token_embed(table, vocab, tokens, pos, out, n, L, D, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_influence_head_f32(const float* h, const float* Wout, const float* bout, float* w, int rows, int D, int nw, void* stream) {
    if (rows == 0) return MMDM_OK;
    if (!h || !Wout || !bout || !w || rows < 0 || D <= 0 || nw <= 0 || nw > 23)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_influence_head_f32: bad arguments rows=%d D=%d nw=%d", rows, D, nw);
    hipLaunchKernelGGL(influence_head_kernel, dim3((rows + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), h, Wout, bout, w, rows, D, nw);
    return mmdm_check_launch("influence_head");
}

// Diagnostic entry points (include/mmdm.h): every row operation in either build, for tests/test_gpu_rowops.py.  Argument checks only -- the launch code is the
// table's, i.e. what the handles run.  build: 0 = this object's kernels (the bits of mmdm_layernorm_f32), 1 = the second build's (no packed-fp32
// instructions, DPP reductions: what a precision 1-3 handle runs).
static const mmdm_rowops* rowops_of(int build, const char* who) {
    if (build != 0 && build != 1) { mmdm_set_error(MMDM_ERR_ARG, "%s: build must be 0 or 1", who); return nullptr; }
    return build ? &mmdm_rowops_tab_nopk : &mmdm_rowops_tab;
}

// planes == NULL: the plain LayerNorm of that build
extern "C" int mmdm_layernorm_split(const float* x, const float* gamma, const float* beta, float* out, void* planes, int64_t plane_stride, int rows, int D, float eps,
                                    int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_layernorm_split");
    if (!ro) return MMDM_ERR_ARG;
    if (!planes) return ro->layernorm(x, gamma, beta, out, rows, D, eps, stream);
    return ro->layernorm_planes(x, gamma, beta, out, planes, plane_stride, rows, D, eps, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_adaln(const float* h, const float* ss, int ss_ld, int ss_rows, void* out, int out_mode, float* row_scale, int nseq, int T, int D,
                                const int* row_seq, int rows_rag, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_adaln");
    if (!ro) return MMDM_ERR_ARG;
    if (out_mode < 0 || out_mode > 3) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_adaln: output mode must be 0 (fp32), 1 (bf16), 2 (two fp16 planes) or 3 (fp8 + row_scale)");
    if (out_mode == 3 && !row_scale) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_adaln: null row_scale");
    if (row_seq && rows_rag < 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_adaln: rows_rag=%d", rows_rag);
    return ro->adaln(h, ss, ss_ld, ss_rows, out, out_mode, row_scale, nseq, T, D, stream, row_seq, rows_rag);
}

extern "C" int mmdm_rowop_cond_silu(const float* time_tab, const int* step_idx, const float* txt, void* out, int planes, int64_t plane_stride, int rows, int D,
                                    int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_cond_silu");
    if (!ro) return MMDM_ERR_ARG;
    if (!planes) return ro->cond_silu(time_tab, step_idx, txt, static_cast<float*>(out), rows, D, stream);
    if (rows == 0) return MMDM_OK;
    if (!time_tab || !step_idx || !txt || !out || rows < 0 || D <= 0 || plane_stride < (int64_t)rows * D)
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_cond_silu: bad arguments rows=%d D=%d plane stride=%lld", rows, D, (long long)plane_stride);
    return ro->cond_silu_planes(time_tab, step_idx, txt, static_cast<_Float16*>(out), (size_t)plane_stride, rows, D, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_mean_time(const float* h, float* out, int nseq, int T, const int* seq_off, const int* seq_len, int D, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_mean_time");
    if (!ro) return MMDM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!seq_off && !seq_len) return ro->mean_time(h, out, mmdm_rows{nseq, T}, D, st);
    if (nseq == 0) return MMDM_OK;
    if (!h || !out || !seq_off || !seq_len || nseq < 0 || D <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_mean_time: bad arguments (ragged: seq_off AND seq_len)");
    return ro->mean_time(h, out, mmdm_rows{nseq, 0, nullptr, nullptr, seq_off, seq_len}, D, st);
}

extern "C" int mmdm_rowop_mdm_pack(const float* src, const float* cond, int ldc, const float* time_tab, const int* step_idx, const float* pe, float* dst, void* planes,
                                   int64_t plane_stride, int nseq, int T, int D, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_mdm_pack");
    if (!ro) return MMDM_ERR_ARG;
    if (nseq == 0) return MMDM_OK;
    if (!src || !cond || !time_tab || !step_idx || !pe || !dst || nseq < 0 || T < 0 || D <= 0 || ldc < D || (planes && plane_stride < (int64_t)nseq * (T + 1) * D))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_mdm_pack: bad arguments nseq=%d T=%d D=%d ldc=%d", nseq, T, D, ldc);
    return ro->mdm_pack(src, cond, ldc, time_tab, step_idx, pe, dst, planes, plane_stride, mmdm_rows{nseq, T}, 0, D, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_mdm_unpack(const float* src, float* dst, int nseq, int T, int D, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_mdm_unpack");
    if (!ro) return MMDM_ERR_ARG;
    if (nseq == 0 || T == 0) return MMDM_OK;
    if (!src || !dst || nseq < 0 || T < 0 || D <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_mdm_unpack: bad arguments nseq=%d T=%d D=%d", nseq, T, D);
    return ro->mdm_unpack(src, dst, mmdm_rows{nseq, T}, D, static_cast<hipStream_t>(stream));
}

// the two row spaces of a ragged batch as the caller's device arrays (kernels.h mmdm_rag): frame rows fr_*, token rows tk_*
#define ROWOP_RAG_CHECK(what)                                                                                                                              \
    if (!fr_row_item || !fr_row_pos || !fr_item_off || !fr_item_len || !tk_row_item || !tk_row_pos || !tk_item_off || !tk_item_len || B <= 0 ||          \
        B > MMDM_RAG_MAX_ITEMS || fr_rows <= 0 || tk_rows <= 0)                                                                                            \
        return mmdm_set_error(MMDM_ERR_ARG, what ": bad row maps B=%d frame rows=%d token rows=%d", B, fr_rows, tk_rows);                                \
    const mmdm_rag fr{fr_row_item, fr_row_pos, fr_item_off, fr_item_len, B, fr_rows}, tk{tk_row_item, tk_row_pos, tk_item_off, tk_item_len, B, tk_rows}

extern "C" int mmdm_rowop_mdm_pack_rag(const float* src, const float* cond, int ldc, const float* time_tab, const int* step_idx, const float* pe, float* dst, void* planes,
                                       int64_t plane_stride, int groups, int gpp, int D, int B, int fr_rows, const int* fr_row_item, const int* fr_row_pos,
                                       const int* fr_item_off, const int* fr_item_len, int tk_rows, const int* tk_row_item, const int* tk_row_pos,
                                       const int* tk_item_off, const int* tk_item_len, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_mdm_pack_rag");
    if (!ro) return MMDM_ERR_ARG;
    if (groups == 0) return MMDM_OK;
    ROWOP_RAG_CHECK("mmdm_rowop_mdm_pack_rag");
    if (!src || !cond || !time_tab || !step_idx || !pe || !dst || groups < 0 || gpp <= 0 || D <= 0 || ldc < (groups + gpp - 1) / gpp * D ||
        (planes && plane_stride < (int64_t)groups * tk_rows * D))
        return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_mdm_pack_rag: bad arguments groups=%d gpp=%d D=%d ldc=%d", groups, gpp, D, ldc);
    return ro->mdm_pack(src, cond, ldc, time_tab, step_idx, pe, dst, planes, plane_stride, mmdm_rows{groups * B, 0, &fr, &tk}, gpp, D, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_mdm_unpack_rag(const float* src, float* dst, int groups, int D, int B, int fr_rows, const int* fr_row_item, const int* fr_row_pos,
                                         const int* fr_item_off, const int* fr_item_len, int tk_rows, const int* tk_row_item, const int* tk_row_pos,
                                         const int* tk_item_off, const int* tk_item_len, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_mdm_unpack_rag");
    if (!ro) return MMDM_ERR_ARG;
    if (groups == 0) return MMDM_OK;
    ROWOP_RAG_CHECK("mmdm_rowop_mdm_unpack_rag");
    if (!src || !dst || groups < 0 || D <= 0) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_mdm_unpack_rag: bad arguments groups=%d D=%d", groups, D);
    return ro->mdm_unpack(src, dst, mmdm_rows{groups * B, 0, &fr, &tk}, D, static_cast<hipStream_t>(stream));
}
#undef ROWOP_RAG_CHECK

// The InterCLIP evaluator's row operations (include/mmdm.h): argument checks are the launchers' own
extern "C" int mmdm_rowop_motion_pack(const float* motions, int64_t item_stride, int row_stride, int Tpad, int npers, float* A, int lda, int Kp, int nseq,
                                      const int* seq_off, const int* seq_len, int max_len, int total_rows, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_motion_pack");
    if (!ro) return MMDM_ERR_ARG;
    return ro->motion_pack(motions, item_stride, row_stride, Tpad, npers, A, nullptr, 0, lda, Kp, nseq, seq_off, seq_len, max_len, total_rows, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_motion_pack_split(const float* motions, int64_t item_stride, int row_stride, int Tpad, int npers, void* planes, int lda, int64_t plane_stride,
                                            int Kp, int nseq, const int* seq_off, const int* seq_len, int max_len, int total_rows, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_motion_pack_split");
    if (!ro) return MMDM_ERR_ARG;
    if (nseq != 0 && !planes) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_pack_split: null planes");
    return ro->motion_pack(motions, item_stride, row_stride, Tpad, npers, nullptr, planes, plane_stride, lda, Kp, nseq, seq_off, seq_len, max_len, total_rows,
                           static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_motion_tokens(float* h, const float* query_token, const float* pe, int pe_rows, int D, int nseq, const int* seq_off, const int* seq_len,
                                        int max_len, int total_rows, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_motion_tokens");
    if (!ro) return MMDM_ERR_ARG;
    return ro->motion_tokens(h, nullptr, 0, query_token, pe, pe_rows, D, nseq, seq_off, seq_len, max_len, total_rows, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_motion_tokens_split(float* h, void* planes, int64_t plane_stride, const float* query_token, const float* pe, int pe_rows, int D, int nseq,
                                              const int* seq_off, const int* seq_len, int max_len, int total_rows, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_motion_tokens_split");
    if (!ro) return MMDM_ERR_ARG;
    if (nseq != 0 && !planes) return mmdm_set_error(MMDM_ERR_ARG, "mmdm_rowop_motion_tokens_split: null planes");
    return ro->motion_tokens(h, planes, plane_stride, query_token, pe, pe_rows, D, nseq, seq_off, seq_len, max_len, total_rows, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_token_embed(const float* table, int vocab, const int* tokens, const float* pos, float* out, int n, int L, int D, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_token_embed");
    if (!ro) return MMDM_ERR_ARG;
    return ro->token_embed(table, vocab, tokens, pos, out, n, L, D, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_l2_normalize_rows_f32(const float* x, const float* scale, float* out, int rows, int D, void* stream) {
    return l2_normalize(x, scale, out, rows, D, static_cast<hipStream_t>(stream));
}

extern "C" int mmdm_rowop_l2_normalize(const float* x, const float* scale, float* out, int rows, int D, int build, void* stream) {
    const mmdm_rowops* ro = rowops_of(build, "mmdm_rowop_l2_normalize");
    if (!ro) return MMDM_ERR_ARG;
    return ro->l2_normalize(x, scale, out, rows, D, static_cast<hipStream_t>(stream));
}
#endif

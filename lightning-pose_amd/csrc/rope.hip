// What the DINOv3 backbones ("vits_dinov3" / "vitb_dinov3", transformers DINOv3ViTModel) add to the ViT glue of vit.hip: the rotary position
// embedding of the patch tokens' queries and keys, and the token assembly with register tokens.  gfx950; the bf16 product forms and the fp32
// validation forms are the same templates (ElemT = bf16 bits / float), as vit_mv.h does for the multi-view assembly.
//
// Rotation (DINOv3ViTAttention -> apply_rotary_pos_emb, head width 64): for a patch token p and d < 32,
//     out[d]      = x[d]      * cos[p][d] - x[d + 32] * sin[p][d]
//     out[d + 32] = x[d + 32] * cos[p][d] + x[d]      * sin[p][d]
// on the Q and K columns of the fused qkv rows, in place; the `n_prefix` leading rows of every sequence ([CLS], registers) and the V columns
// are neither read nor written.  Two fp32 products and one fp32 sum / difference per element, never a fused multiply-add, then ONE rounding to
// bf16: the result is the float32 evaluation of the formula as written.  The backward pass is the transposed rotation (sin -> -sin) on dQ / dK.
//
// Lanes: four per (token, q-or-k, head) slot; lane j of a slot holds columns [8j, 8j + 8) and [32 + 8j, 40 + 8j) - two 16-byte loads and two
// 16-byte stores in the bf16 form - so the 16 lanes of four neighbouring heads cover 512 contiguous bytes and a token's 2 * nh * 128 bytes
// stay contiguous across a wave.  The table row of a patch (cos[0:32] | sin[0:32], 256 B) is shared by every head, q and k and every image
// that uses that table: it stays in L2.  No LDS, no atomics, no reduction: every run writes the same bits.
#include "lp_common.h"

namespace lp {

__device__ __forceinline__ void rope_load8(const unsigned short* p, float (&f)[8]) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = bf16_to_f32(v[i]);
}
__device__ __forceinline__ void rope_load8(const float* p, float (&f)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = a[i], f[4 + i] = b[i];
}
__device__ __forceinline__ void rope_store8(unsigned short* p, const float (&f)[8]) { *reinterpret_cast<u16x8*>(p) = pack_bf16x8(f); }
__device__ __forceinline__ void rope_store8(float* p, const float (&f)[8]) {
    const f32x4 a = {f[0], f[1], f[2], f[3]}, b = {f[4], f[5], f[6], f[7]};
    *reinterpret_cast<f32x4*>(p) = a;
    *reinterpret_cast<f32x4*>(p + 4) = b;
}

// a * c + b * s as two products and one sum (device code is compiled with -ffp-contract=fast-honor-pragmas)
__device__ __forceinline__ float rope_mix(float a, float c, float b, float s) {
#pragma clang fp contract(off)
    const float t0 = a * c, t1 = b * s;
    return t0 + t1;
}

// BWD: the transposed rotation.  `tab_of_seq` == nullptr: every sequence uses table 0; an index outside [0, n_tab) is clamped into it (the
// launch cannot read the device array, and a stray index must not leave the table)
template <typename ElemT, bool BWD>
__global__ __launch_bounds__(256) void rope_kernel(ElemT* __restrict__ qkv, int ld, int k_off, const float* __restrict__ table,
                                                   const int* __restrict__ tab_of_seq, int n_tab, int B, int T, int n_prefix, int nh) {
    const int Np = T - n_prefix;
    const size_t total = (size_t)B * Np * 2 * nh * 4;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
        const int j = (int)(q & 3);
        size_t s = q >> 2;
        const int h = (int)(s % nh);
        s /= nh;
        const int qk = (int)(s & 1);
        s >>= 1;
        const int p = (int)(s % Np), b = (int)(s / Np);
        int ti = tab_of_seq != nullptr ? tab_of_seq[b] : 0;
        ti = ti < 0 ? 0 : (ti >= n_tab ? n_tab - 1 : ti);
        const float* tr = table + ((size_t)ti * Np + p) * 64 + 8 * j;
        ElemT* xr = qkv + ((size_t)b * T + n_prefix + p) * ld + (qk ? k_off : 0) + h * 64 + 8 * j;
        float lo[8], hi[8], c[8], sn[8], olo[8], ohi[8];
        rope_load8(xr, lo);
        rope_load8(xr + 32, hi);
        rope_load8(tr, c);
        rope_load8(tr + 32, sn);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float sg = BWD ? -sn[i] : sn[i];
            olo[i] = rope_mix(lo[i], c[i], hi[i], -sg);
            ohi[i] = rope_mix(hi[i], c[i], lo[i], sg);
        }
        rope_store8(xr, olo);
        rope_store8(xr + 32, ohi);
    }
}

template <typename ElemT, bool BWD>
inline int rope_launch(ElemT* qkv, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix, int nh,
                       int head_dim, hipStream_t stream) {
    LP_REQUIRE(qkv && table && n_tab > 0 && B > 0 && T > 0 && nh > 0 && head_dim > 0 && n_prefix >= 0 && n_prefix <= T && ld > 0 && k_off >= 0);
    if (head_dim != 64) return LP_ERR_UNSUPPORTED;
    LP_REQUIRE(k_off >= nh * 64 && k_off + nh * 64 <= ld);   // Q and K are disjoint column blocks inside the row
    constexpr int kAlign = 16 / (int)sizeof(ElemT);           // elements per 16 bytes
    if (ld % kAlign != 0 || k_off % kAlign != 0 || (uintptr_t)qkv % 16 != 0 || (uintptr_t)table % 16 != 0) return LP_ERR_UNSUPPORTED;
    if (n_prefix == T) return LP_OK;   // no patch rows
    size_t blocks = ((size_t)B * (T - n_prefix) * 2 * nh * 4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL((rope_kernel<ElemT, BWD>), dim3((unsigned)blocks), dim3(256), 0, stream, qkv, ld, k_off, table, tab_of_seq, n_tab, B, T,
                       n_prefix, nh);
    return launch_status();
}

// ---- tokens: x[b][0] = cls;  x[b][1 + r] = reg[r];  x[b][1 + R + p] = float(patch[b * Np + p])  (nothing is added: no position table) ------
template <typename PatchT>
__global__ __launch_bounds__(256) void vit_reg_tokens_fwd_kernel(const PatchT* __restrict__ patch, const float* __restrict__ cls,
                                                                 const float* __restrict__ reg, int B, int R, int Np, int D,
                                                                 float* __restrict__ x) {
    const int T = 1 + R + Np, chunks = D >> 3;
    const size_t total = (size_t)B * T * chunks;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
        const int ch = (int)(q % chunks);
        const size_t row = q / chunks;
        const int t = (int)(row % T), b = (int)(row / T);
        float v[8];
        if (t == 0) {
            rope_load8(cls + ch * 8, v);
        } else if (t <= R) {
            rope_load8(reg + (size_t)(t - 1) * D + ch * 8, v);
        } else {
            rope_load8(patch + ((size_t)b * Np + t - 1 - R) * D + ch * 8, v);
        }
        rope_store8(x + row * D + ch * 8, v);
    }
}

// backward: dpatch[b][p] = dx[b][1 + R + p] (rounded to bf16 in the product form);  dprefix[t] = sum_b dx[b][t] for t <= R, images in
// ascending order in one thread - WRITTEN, not accumulated; row 0 is d cls, rows 1 .. R are d reg
template <typename PatchT>
__global__ __launch_bounds__(256) void vit_reg_tokens_bwd_kernel(const float* __restrict__ dx, int B, int R, int Np, int D,
                                                                 PatchT* __restrict__ dpatch, float* __restrict__ dcls,
                                                                 float* __restrict__ dreg) {
    const int T = 1 + R + Np, chunks = D >> 3;
    const int total = T * chunks;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < total; q += gridDim.x * 256) {
        const int ch = q % chunks, t = q / chunks;
        if (t > R) {
            for (int b = 0; b < B; ++b) {
                float v[8];
                rope_load8(dx + ((size_t)b * T + t) * D + ch * 8, v);
                rope_store8(dpatch + ((size_t)b * Np + t - 1 - R) * D + ch * 8, v);
            }
            continue;
        }
        float s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = 0.f;
        for (int b = 0; b < B; ++b) {
            float v[8];
            rope_load8(dx + ((size_t)b * T + t) * D + ch * 8, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] += v[i];
        }
        rope_store8(t == 0 ? dcls + ch * 8 : dreg + (size_t)(t - 1) * D + ch * 8, s);
    }
}

static int reg_grid(size_t work_items) {
    size_t blocks = (work_items + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    return blocks < 1 ? 1 : (int)blocks;
}

template <typename PatchT>
inline int reg_tokens_fwd_launch(const PatchT* patch, const float* cls, const float* reg, int B, int R, int Np, int D, float* x,
                                 hipStream_t stream) {
    LP_REQUIRE(patch && cls && x && B > 0 && R >= 0 && Np > 0 && D > 0 && (R == 0 || reg != nullptr));
    if (D % 8 != 0) return LP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vit_reg_tokens_fwd_kernel<PatchT>, dim3(reg_grid((size_t)B * (1 + R + Np) * (D / 8))), dim3(256), 0, stream, patch, cls,
                       reg, B, R, Np, D, x);
    return launch_status();
}

template <typename PatchT>
inline int reg_tokens_bwd_launch(const float* dx, int B, int R, int Np, int D, PatchT* dpatch, float* dcls, float* dreg, hipStream_t stream) {
    LP_REQUIRE(dx && dpatch && dcls && B > 0 && R >= 0 && Np > 0 && D > 0 && (R == 0 || dreg != nullptr));
    if (D % 8 != 0) return LP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vit_reg_tokens_bwd_kernel<PatchT>, dim3(reg_grid((size_t)(1 + R + Np) * (D / 8))), dim3(256), 0, stream, dx, B, R, Np, D,
                       dpatch, dcls, dreg);
    return launch_status();
}

}  // namespace lp

extern "C" int lp_rope_fwd(void* qkv_bf16, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix,
                           int nh, int head_dim, lp_stream_t stream) {
    return lp::rope_launch<unsigned short, false>((unsigned short*)qkv_bf16, ld, k_off, table, tab_of_seq, n_tab, B, T, n_prefix, nh, head_dim,
                                                  (hipStream_t)stream);
}

extern "C" int lp_rope_bwd(void* dqkv_bf16, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix,
                           int nh, int head_dim, lp_stream_t stream) {
    return lp::rope_launch<unsigned short, true>((unsigned short*)dqkv_bf16, ld, k_off, table, tab_of_seq, n_tab, B, T, n_prefix, nh, head_dim,
                                                 (hipStream_t)stream);
}

extern "C" int lp_f32_rope_fwd(float* qkv, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix,
                               int nh, int head_dim, lp_stream_t stream) {
    return lp::rope_launch<float, false>(qkv, ld, k_off, table, tab_of_seq, n_tab, B, T, n_prefix, nh, head_dim, (hipStream_t)stream);
}

extern "C" int lp_f32_rope_bwd(float* dqkv, int ld, int k_off, const float* table, const int* tab_of_seq, int n_tab, int B, int T, int n_prefix,
                               int nh, int head_dim, lp_stream_t stream) {
    return lp::rope_launch<float, true>(dqkv, ld, k_off, table, tab_of_seq, n_tab, B, T, n_prefix, nh, head_dim, (hipStream_t)stream);
}

extern "C" int lp_vit_reg_tokens_fwd(const void* patch_bf16, const float* cls, const float* reg, int B, int R, int Np, int D, float* x,
                                     lp_stream_t stream) {
    return lp::reg_tokens_fwd_launch((const unsigned short*)patch_bf16, cls, reg, B, R, Np, D, x, (hipStream_t)stream);
}

extern "C" int lp_vit_reg_tokens_bwd(const float* dx, int B, int R, int Np, int D, void* dpatch_bf16, float* dcls, float* dreg,
                                     lp_stream_t stream) {
    return lp::reg_tokens_bwd_launch(dx, B, R, Np, D, (unsigned short*)dpatch_bf16, dcls, dreg, (hipStream_t)stream);
}

extern "C" int lp_f32_vit_reg_tokens_fwd(const float* patch, const float* cls, const float* reg, int B, int R, int Np, int D, float* x,
                                         lp_stream_t stream) {
    return lp::reg_tokens_fwd_launch(patch, cls, reg, B, R, Np, D, x, (hipStream_t)stream);
}

extern "C" int lp_f32_vit_reg_tokens_bwd(const float* dx, int B, int R, int Np, int D, float* dpatch, float* dcls, float* dreg,
                                         lp_stream_t stream) {
    return lp::reg_tokens_bwd_launch(dx, B, R, Np, D, dpatch, dcls, dreg, (hipStream_t)stream);
}

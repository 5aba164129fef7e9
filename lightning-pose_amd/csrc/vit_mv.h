// Token assembly of the multi-view transformer tracker (reference models/heatmap_tracker_multiview.py:143-223, forward_vit): the patch
// embeddings of the V views of a sample become ONE sequence of V * Np tokens - no [CLS] row - and every token of view v carries the learned
// embedding view[v] on top of its position embedding.  Included by vit.hip (PatchT = bf16 bits, the product path) and vit_f32.hip (float).
//
// Row r = (b * V + v) * Np + p of the patch tensor IS row b * (V * Np) + v * Np + p of the residual stream, so both kernels keep the row
// index and only decode (v, p) from it.
//
//   forward    x[r][:] = (patch[r][:] + pos[1 + p][:]) + view[v][:]          (fp32; this order of the two additions, HF's own)
//   backward   dpatch[r] = dx[r] (rounded to bf16 in the product path),  dpos[1 + p] = sum_{b,v} dx,  dview[v] = sum_{b,p} dx
//
// The backward is one pass over dx and a two-level reduction without floating-point atomics:
//   level 1  a workgroup of 256 threads = 16 row slots x 16 column chunks (float4) owns (view v, a group of `gb` samples, 16 patch rows,
//            64 columns).  A thread reads its row p of each sample of the group (independent 16-B loads), stores dpatch and keeps ONE
//            running float4: summed over the group it is the workgroup's dpos partial for (v, group, p) - written straight to the workspace -
//            and, summed over the 16 row slots (two wave shuffles, then 4 wave partials through LDS, added in wave order), the workgroup's
//            dview partial for (v, group, row tile).
//   level 2  one small launch adds the partials in a fixed order: dpos[1 + p] over (v, group) ascending; dview[v] over (group, row tile): 16
//            slots each add every 16th partial in ascending order, then the 16 slot sums are added in slot order.
// Every sum has one order that depends on the shape alone: two runs give the same bits.
#pragma once

#include "lp_common.h"

namespace lp {

constexpr int kMvRows = 16;   // patch rows per workgroup (one per row slot)
constexpr int kMvCols = 64;   // columns per workgroup (16 float4 chunks)

struct MvPlan {
    int gb;    // samples per group
    int nbg;   // groups
    int npt;   // row tiles
};

// enough workgroups to fill the chip (4 per CU) before samples are summed serially inside one
inline MvPlan mv_plan(int B, int V, int Np, int D) {
    MvPlan pl;
    pl.npt = (Np + kMvRows - 1) / kMvRows;
    const long long base = (long long)V * pl.npt * (D / kMvCols);
    long long want = (1024 + base - 1) / base;
    if (want > B) want = B;
    if (want < 1) want = 1;
    pl.gb = (int)((B + want - 1) / want);
    pl.nbg = (B + pl.gb - 1) / pl.gb;
    return pl;
}

// workspace: dpos partials [V][nbg][Np][D], then dview partials [V][nbg][npt][D]
inline size_t mv_ws_floats(const MvPlan& pl, int V, int Np, int D) {
    return (size_t)V * pl.nbg * ((size_t)Np + pl.npt) * D;
}

__device__ __forceinline__ void mv_load8(const unsigned short* p, float (&f)[8]) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = bf16_to_f32(v[i]);
}
__device__ __forceinline__ void mv_load8(const float* p, float (&f)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = a[i], f[4 + i] = b[i];
}
__device__ __forceinline__ void mv_store4(unsigned short* p, const f32x4& v) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
    *reinterpret_cast<u32x2_t*>(p) = u32x2_t{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}
__device__ __forceinline__ void mv_store4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }

template <typename PatchT>
__global__ __launch_bounds__(256) void vit_mv_tokens_fwd_kernel(const PatchT* __restrict__ patch, const float* __restrict__ pos,
                                                                const float* __restrict__ view, int B, int V, int Np, int D,
                                                                float* __restrict__ x) {
    const int chunks = D >> 3;
    const size_t total = (size_t)B * V * Np * chunks;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
        const int ch = (int)(q % chunks);
        const size_t row = q / chunks;
        const int p = (int)(row % Np), v = (int)((row / Np) % V);
        float a[8], e[8], w[8];
        mv_load8(patch + row * D + ch * 8, a);
        mv_load8(pos + (size_t)(1 + p) * D + ch * 8, e);
        mv_load8(view + (size_t)v * D + ch * 8, w);
        f32x4 lo, hi;
#pragma unroll
        for (int i = 0; i < 4; ++i) lo[i] = (a[i] + e[i]) + w[i], hi[i] = (a[4 + i] + e[4 + i]) + w[4 + i];
        float* dst = x + row * D + ch * 8;
        *reinterpret_cast<f32x4*>(dst) = lo;
        *reinterpret_cast<f32x4*>(dst + 4) = hi;
    }
}

// level 1.  grid = (npt, D / 64, V * nbg)
template <typename PatchT>
__global__ __launch_bounds__(256) void vit_mv_tokens_bwd_kernel(const float* __restrict__ dx, int B, int V, int Np, int D, int gb,
                                                                PatchT* __restrict__ dpatch, float* __restrict__ ws_pos,
                                                                float* __restrict__ ws_view) {
    __shared__ float part[4][kMvCols];
    const int cc = threadIdx.x & 15, rs = threadIdx.x >> 4, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbg = (B + gb - 1) / gb;
    const int pt = blockIdx.x, v = blockIdx.z / nbg, bg = blockIdx.z % nbg;
    const int p = pt * kMvRows + rs, col = blockIdx.y * kMvCols + cc * 4;
    const int b0 = bg * gb, b1 = min(B, b0 + gb);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (p < Np) {
#pragma unroll 4
        for (int b = b0; b < b1; ++b) {
            const size_t off = (((size_t)b * V + v) * Np + p) * D + col;
            const f32x4 g = *reinterpret_cast<const f32x4*>(dx + off);
            mv_store4(dpatch + off, g);
            acc += g;
        }
        *reinterpret_cast<f32x4*>(ws_pos + (((size_t)v * nbg + bg) * Np + p) * D + col) = acc;
    }
    // the 16 row slots of this column chunk: 4 inside the wave (lanes cc, 16 + cc, 32 + cc, 48 + cc), then the 4 waves
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float s = acc[i];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        acc[i] = s;
    }
    if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) part[wave][cc * 4 + i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < kMvCols) {
        const int c = threadIdx.x;
        const float s = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
        ws_view[(((size_t)v * nbg + bg) * gridDim.x + pt) * D + blockIdx.y * kMvCols + c] = s;
    }
}

// level 2.  blocks [0, pos_blocks): dpos rows 0 .. Np (row 0, the [CLS] position, is zero), one float4 per thread;
// blocks [pos_blocks, pos_blocks + V * D / 64): dview[v], 64 columns per block
static __global__ __launch_bounds__(256) void vit_mv_tokens_combine_kernel(const float* __restrict__ ws_pos, const float* __restrict__ ws_view, int V,
                                                                    int Np, int D, int nbg, int npt, int pos_blocks,
                                                                    float* __restrict__ dpos, float* __restrict__ dview) {
    __shared__ float slot[16][kMvCols];
    if ((int)blockIdx.x < pos_blocks) {
        const int chunks = D >> 2;
        const int q = blockIdx.x * 256 + threadIdx.x;
        if (q >= (Np + 1) * chunks) return;
        const int row = q / chunks, col = (q % chunks) * 4;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (row > 0)
            for (int j = 0; j < V * nbg; ++j) s += *reinterpret_cast<const f32x4*>(ws_pos + ((size_t)j * Np + row - 1) * D + col);
        *reinterpret_cast<f32x4*>(dpos + (size_t)row * D + col) = s;
        return;
    }
    const int blk = blockIdx.x - pos_blocks, groups = D / kMvCols;
    const int v = blk / groups, col = (blk % groups) * kMvCols;
    const int cc = threadIdx.x & 15, sl = threadIdx.x >> 4, n = nbg * npt;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int j = sl; j < n; j += 16) s += *reinterpret_cast<const f32x4*>(ws_view + ((size_t)v * n + j) * D + col + cc * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) slot[sl][cc * 4 + i] = s[i];
    __syncthreads();
    if (threadIdx.x < kMvCols) {
        float t = slot[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < 16; ++i) t += slot[i][threadIdx.x];
        dview[(size_t)v * D + col + threadIdx.x] = t;
    }
}

template <typename PatchT>
inline int mv_tokens_fwd_launch(const PatchT* patch, const float* pos, const float* view, int B, int V, int Np, int D, float* x,
                                hipStream_t stream) {
    LP_REQUIRE(patch && pos && view && x && B > 0 && V > 0 && Np > 0 && D > 0);
    if (D % kMvCols != 0) return LP_ERR_UNSUPPORTED;
    size_t blocks = ((size_t)B * V * Np * (D / 8) + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(vit_mv_tokens_fwd_kernel<PatchT>, dim3((unsigned)blocks), dim3(256), 0, stream, patch, pos, view, B, V, Np, D, x);
    return launch_status();
}

template <typename PatchT>
inline int mv_tokens_bwd_launch(const float* dx, int B, int V, int Np, int D, PatchT* dpatch, float* dpos, float* dview, float* ws,
                                size_t ws_bytes, hipStream_t stream) {
    LP_REQUIRE(dx && dpatch && dpos && dview && ws && B > 0 && V > 0 && Np > 0 && D > 0);
    if (D % kMvCols != 0) return LP_ERR_UNSUPPORTED;
    const MvPlan pl = mv_plan(B, V, Np, D);
    if ((long long)V * pl.nbg > 65535 || D / kMvCols > 65535) return LP_ERR_UNSUPPORTED;   // (grid.z / grid.y)
    LP_REQUIRE(ws_bytes >= mv_ws_floats(pl, V, Np, D) * sizeof(float));
    float* ws_pos = ws;
    float* ws_view = ws + (size_t)V * pl.nbg * Np * D;
    hipLaunchKernelGGL(vit_mv_tokens_bwd_kernel<PatchT>, dim3(pl.npt, D / kMvCols, V * pl.nbg), dim3(256), 0, stream, dx, B, V, Np, D, pl.gb,
                       dpatch, ws_pos, ws_view);
    const int pos_blocks = ((Np + 1) * (D / 4) + 255) / 256;
    hipLaunchKernelGGL(vit_mv_tokens_combine_kernel, dim3(pos_blocks + V * (D / kMvCols)), dim3(256), 0, stream, ws_pos, ws_view, V, Np, D,
                       pl.nbg, pl.npt, pos_blocks, dpos, dview);
    return launch_status();
}

}  // namespace lp

// What the SAM backbone ("vitb_sam", transformers SamVisionEncoder without relative positions and without its neck) adds to the ViT glue of
// vit.hip: windowed attention.  Eight of ViT-B's twelve layers attend inside ws x ws windows of the token grid, zero-padded on the bottom
// and right to multiples of the window.  The attention kernels stay as they are - they see B * nW sequences of ws * ws tokens - and the two
// moves below take a tensor between the grid layout [B][gh][gw][cols] (rows with a pitch) and the window layout [B * nW][ws * ws][cols]
// (dense), window b * nW + wy * nWx + wx, token ty * ws + tx  <->  grid position (wy * ws + ty, wx * ws + tx):
//     partition     grid -> windows; the rows of pad positions are filled from a `cols`-long vector (the fused qkv tensor: a padded token is
//                   zero AFTER the LayerNorm, so its q, k, v are the qkv bias, and it takes part in every soft-max of its window) or with
//                   zeros (gradients)
//     un-partition  windows -> grid; the pad rows are dropped - or, with `pad_colsum`, their per-column sums are ADDED to that fp32 vector:
//                   the pad rows' dK / dV are gradient of the qkv bias
// Both are pure moves in 16-byte pieces (NaN payloads and -0.0 survive); a wave takes one row, so the index arithmetic is per row, and its
// lanes cover 1 KiB of the row per pass.  bf16 product forms and fp32 validation forms are the same templates.
//
// The pad-row sums need no atomics and no workspace: the un-partition launch carries extra workgroups, each owning 4 pieces of the row (32
// bf16 / 16 fp32 columns).  The pad positions are enumerated directly (per image: the strip right of the grid row by row, then the strip
// below it), so no lane visits a real row; each of the 64 row slots takes the pad positions 64 apart in ascending order - eight loads in
// flight, added in that order in fp32 - the slots are then added in ascending order by one thread per piece, and the total is added to
// pad_colsum once.  The order is fixed by the shapes alone: every run gives the same bits.
//
// Also here, because SAM has neither a [CLS] token nor a final LayerNorm: the token assembly x = patch embedding + position table, and the
// final residual add that hands the last layer's stream to the head (and the head's gradient back into the stream gradient).
#include "lp_common.h"

namespace lp {

struct WinGeom {
    int B, gh, gw, ws, nwy, nwx;
};

// window-layout row -> grid-layout row, -1 for a pad position
__device__ __forceinline__ long long win_grid_row(long long r, const WinGeom& g) {
    const int t2 = g.ws * g.ws, nW = g.nwy * g.nwx;
    const long long w = r / t2;
    const int t = (int)(r - w * t2);
    const int ty = t / g.ws, tx = t - ty * g.ws;
    const long long b = w / nW;
    const int wi = (int)(w - b * nW);
    const int wy = wi / g.nwx, wx = wi - wy * g.nwx;
    const int gy = wy * g.ws + ty, gx = wx * g.ws + tx;
    if (gy >= g.gh || gx >= g.gw) return -1;
    return (b * g.gh + gy) * g.gw + gx;
}

// grid-layout row -> window-layout row
__device__ __forceinline__ long long win_window_row(long long s, const WinGeom& g) {
    const long long bg = s / g.gw;
    const int gx = (int)(s - bg * g.gw);
    const long long b = bg / g.gh;
    const int gy = (int)(bg - b * g.gh);
    const int wy = gy / g.ws, ty = gy - wy * g.ws, wx = gx / g.ws, tx = gx - wx * g.ws;
    return ((b * g.nwy + wy) * g.nwx + wx) * (long long)(g.ws * g.ws) + ty * g.ws + tx;
}

// the j-th pad position (image, then the right strip row by row, then the bottom strip) -> window-layout row.  `right` = padded width - gw,
// `n_right` = gh * right, `per_image` = pad positions of one image
__device__ __forceinline__ long long win_pad_row(long long j, const WinGeom& g, int per_image, int right, int n_right) {
    const long long b = j / per_image;
    int r = (int)(j - b * per_image), gy, gx;
    if (r < n_right) {
        gy = r / right;
        gx = g.gw + (r - gy * right);
    } else {
        const int wp = g.nwx * g.ws;
        r -= n_right;
        gy = r / wp;
        gx = r - gy * wp;
        gy += g.gh;
    }
    const int wy = gy / g.ws, ty = gy - wy * g.ws, wx = gx / g.ws, tx = gx - wx * g.ws;
    return ((b * g.nwy + wy) * g.nwx + wx) * (long long)(g.ws * g.ws) + ty * g.ws + tx;
}

// `src` rows ld16 pieces apart; `dst` dense, `chunks` pieces a row.  One wave per window row.
__global__ __launch_bounds__(256) void window_partition_kernel(const u16x8* __restrict__ src, long long ld16, WinGeom g, int chunks,
                                                               const u16x8* __restrict__ fill, u16x8* __restrict__ dst, long long rows) {
    const int lane = threadIdx.x & 63;
    const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * 4) {
        const long long s = win_grid_row(r, g);
        u16x8* d = dst + r * chunks;
        if (s >= 0) {
            const u16x8* p = src + s * ld16;
            for (int ch = lane; ch < chunks; ch += 64) d[ch] = p[ch];
        } else if (fill != nullptr) {
            for (int ch = lane; ch < chunks; ch += 64) d[ch] = fill[ch];
        } else {
            for (int ch = lane; ch < chunks; ch += 64) d[ch] = zero;
        }
    }
}

__device__ __forceinline__ void win_add(const u16x8& v, float (&acc)[8], unsigned short) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += bf16_to_f32(v[i]);
}
__device__ __forceinline__ void win_add(const u16x8& v, float (&acc)[8], float) {
    const f32x4 f = __builtin_bit_cast(f32x4, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += f[i];
}

// workgroups [0, move_blocks): one wave per grid row, src dense (`chunks` pieces a row), dst rows ld16 pieces apart.
// workgroups behind them (pad_colsum != nullptr): the pad rows' column sums, 4 pieces of the row each - thread = (row slot 0 .. 63, piece)
template <typename ElemT>
__global__ __launch_bounds__(256) void window_unpartition_kernel(const u16x8* __restrict__ src, WinGeom g, int chunks, u16x8* __restrict__ dst,
                                                                 long long ld16, long long grid_rows, long long n_pad, int move_blocks,
                                                                 float* __restrict__ pad_colsum) {
    constexpr int kPer = 16 / (int)sizeof(ElemT);   // columns in a piece
    constexpr int kFly = 8;                         // loads in flight per lane
    __shared__ float red[64][4][8];
    if ((int)blockIdx.x < move_blocks) {
        const int lane = threadIdx.x & 63;
        for (long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); s < grid_rows; s += (long long)move_blocks * 4) {
            const u16x8* p = src + win_window_row(s, g) * chunks;
            u16x8* d = dst + s * ld16;
            for (int ch = lane; ch < chunks; ch += 64) d[ch] = p[ch];
        }
        return;
    }
    const int pc = threadIdx.x & 3, slot = threadIdx.x >> 2;
    const int ch = ((int)blockIdx.x - move_blocks) * 4 + pc;
    const int right = g.nwx * g.ws - g.gw, n_right = g.gh * right;
    const int per_image = n_right + (g.nwy * g.ws - g.gh) * (g.nwx * g.ws);
    const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    if (ch < chunks) {
        for (long long j0 = slot; j0 < n_pad; j0 += 64 * kFly) {
            u16x8 v[kFly];
#pragma unroll
            for (int u = 0; u < kFly; ++u) {   // (a slot's tail adds zeros: x + 0 = x)
                const long long j = j0 + 64 * u;
                v[u] = j < n_pad ? src[win_pad_row(j, g, per_image, right, n_right) * chunks + ch] : zero;
            }
#pragma unroll
            for (int u = 0; u < kFly; ++u) win_add(v[u], acc, ElemT{});
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[slot][pc][i] = acc[i];
    __syncthreads();
    if (slot == 0 && ch < chunks) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            float t = 0.f;
            for (int sl = 0; sl < 64; ++sl) t += red[sl][pc][i];
            pad_colsum[ch * kPer + i] += t;
        }
    }
}

static int win_grid(long long work_items, int per_block) {
    long long blocks = (work_items + per_block - 1) / per_block;
    if (blocks > 256 * 16) blocks = 256 * 16;
    return blocks < 1 ? 1 : (int)blocks;
}

// the checks both moves share; *g and *chunks are filled when they pass
template <typename ElemT>
inline int win_check(const void* a, const void* b, const void* opt, int ld, int B, int gh, int gw, int ws, int cols, WinGeom* g, int* chunks) {
    LP_REQUIRE(a && b && B > 0 && gh > 0 && gw > 0 && ws >= 1 && cols > 0 && ld >= cols);
    constexpr int kPer = 16 / (int)sizeof(ElemT);
    if (cols % kPer != 0 || ld % kPer != 0 || (uintptr_t)a % 16 != 0 || (uintptr_t)b % 16 != 0 || (uintptr_t)opt % 16 != 0)
        return LP_ERR_UNSUPPORTED;
    const long long nwy = ((long long)gh + ws - 1) / ws, nwx = ((long long)gw + ws - 1) / ws;
    const long long win_rows = (long long)B * nwy * nwx * ws * ws;   // (ws <= 46340 keeps ws * ws an int; more is refused just below)
    if (ws > 32768 || nwy * nwx * ws * ws >= (1LL << 31) || win_rows >= (1LL << 40)) return LP_ERR_UNSUPPORTED;
    *g = WinGeom{B, gh, gw, ws, (int)nwy, (int)nwx};
    *chunks = cols / kPer;
    return LP_OK;
}

template <typename ElemT>
inline int window_partition_launch(const ElemT* src, int ld_src, int B, int gh, int gw, int ws, int cols, const ElemT* fill, ElemT* dst,
                                   hipStream_t stream) {
    WinGeom g;
    int chunks;
    const int rc = win_check<ElemT>(src, dst, fill, ld_src, B, gh, gw, ws, cols, &g, &chunks);
    if (rc != LP_OK) return rc;
    constexpr int kPer = 16 / (int)sizeof(ElemT);
    const long long rows = (long long)B * g.nwy * g.nwx * ws * ws;
    hipLaunchKernelGGL(window_partition_kernel, dim3(win_grid(rows, 4)), dim3(256), 0, stream, reinterpret_cast<const u16x8*>(src),
                       (long long)(ld_src / kPer), g, chunks, reinterpret_cast<const u16x8*>(fill), reinterpret_cast<u16x8*>(dst), rows);
    return launch_status();
}

template <typename ElemT>
inline int window_unpartition_launch(const ElemT* src, int B, int gh, int gw, int ws, int cols, ElemT* dst, int ld_dst, float* pad_colsum,
                                     hipStream_t stream) {
    WinGeom g;
    int chunks;
    const int rc = win_check<ElemT>(src, dst, nullptr, ld_dst, B, gh, gw, ws, cols, &g, &chunks);   // (pad_colsum: scalar accesses only)
    if (rc != LP_OK) return rc;
    constexpr int kPer = 16 / (int)sizeof(ElemT);
    const long long grid_rows = (long long)B * gh * gw, win_rows = (long long)B * g.nwy * g.nwx * ws * ws;
    const int move_blocks = win_grid(grid_rows, 4);
    const int sum_blocks = (pad_colsum != nullptr && win_rows > grid_rows) ? (chunks + 3) / 4 : 0;   // (no pad rows: nothing to add)
    hipLaunchKernelGGL(window_unpartition_kernel<ElemT>, dim3(move_blocks + sum_blocks), dim3(256), 0, stream,
                       reinterpret_cast<const u16x8*>(src), g, chunks, reinterpret_cast<u16x8*>(dst), (long long)(ld_dst / kPer), grid_rows,
                       win_rows - grid_rows, move_blocks, pad_colsum);
    return launch_status();
}

// ---- tokens without a prefix: x[b][p] = float(patch[b * Np + p]) + pos[p] -------------------------------------------------------------------
__device__ __forceinline__ void win_load8(const unsigned short* p, float (&f)[8]) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = bf16_to_f32(v[i]);
}
__device__ __forceinline__ void win_load8(const float* p, float (&f)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = a[i], f[4 + i] = b[i];
}
__device__ __forceinline__ void win_store8(unsigned short* p, const float (&f)[8]) { *reinterpret_cast<u16x8*>(p) = pack_bf16x8(f); }
__device__ __forceinline__ void win_store8(float* p, const float (&f)[8]) {
    const f32x4 a = {f[0], f[1], f[2], f[3]}, b = {f[4], f[5], f[6], f[7]};
    *reinterpret_cast<f32x4*>(p) = a;
    *reinterpret_cast<f32x4*>(p + 4) = b;
}

template <typename PatchT>
__global__ __launch_bounds__(256) void vit_pos_tokens_fwd_kernel(const PatchT* __restrict__ patch, const float* __restrict__ pos, int B, int Np,
                                                                 int D, float* __restrict__ x) {
    const int chunks = D >> 3;
    const size_t per_image = (size_t)Np * chunks, total = (size_t)B * per_image;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (size_t)gridDim.x * 256) {
        float v[8], e[8];
        win_load8(patch + q * 8, v);
        win_load8(pos + (q % per_image) * 8, e);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += e[i];
        win_store8(x + q * 8, v);
    }
}

// backward: dpatch = dx (rounded to bf16 in the product form);  dpos[p] = sum_b dx[b][p], images in ascending order in one thread - WRITTEN,
// not accumulated, as lp_vit_reg_tokens_bwd does
template <typename PatchT>
__global__ __launch_bounds__(256) void vit_pos_tokens_bwd_kernel(const float* __restrict__ dx, int B, int Np, int D, PatchT* __restrict__ dpatch,
                                                                 float* __restrict__ dpos) {
    const size_t per_image = (size_t)Np * (D >> 3);
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < per_image; q += (size_t)gridDim.x * 256) {
        float s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = 0.f;
        for (int b = 0; b < B; ++b) {
            float v[8];
            win_load8(dx + (b * per_image + q) * 8, v);
            win_store8(dpatch + (b * per_image + q) * 8, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] += v[i];
        }
        win_store8(dpos + q * 8, s);
    }
}

// ---- the last layer's residual add: x_out = x + delta, and (product form) y = bf16(x_out), the features the head reads -------------------
template <typename ElemT, bool WITH_Y>
__global__ __launch_bounds__(256) void resid_out_fwd_kernel(const float* x, const ElemT* __restrict__ delta, size_t chunks, float* x_out,
                                                            unsigned short* __restrict__ y) {
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < chunks; q += (size_t)gridDim.x * 256) {
        float v[8], d[8];
        win_load8(x + q * 8, v);
        win_load8(delta + q * 8, d);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += d[i];
        win_store8(x_out + q * 8, v);
        if (WITH_Y) win_store8(y + q * 8, v);
    }
}

// backward: the stream gradient starts as the head's gradient, dx = float(dy) - WRITTEN
template <typename ElemT>
__global__ __launch_bounds__(256) void resid_out_bwd_kernel(const ElemT* __restrict__ dy, size_t chunks, float* __restrict__ dx) {
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < chunks; q += (size_t)gridDim.x * 256) {
        float v[8];
        win_load8(dy + q * 8, v);
        win_store8(dx + q * 8, v);
    }
}

template <typename PatchT>
inline int pos_tokens_fwd_launch(const PatchT* patch, const float* pos, int B, int Np, int D, float* x, hipStream_t stream) {
    LP_REQUIRE(patch && pos && x && B > 0 && Np > 0 && D > 0);
    if (D % 8 != 0) return LP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vit_pos_tokens_fwd_kernel<PatchT>, dim3(win_grid((long long)B * Np * (D / 8), 256)), dim3(256), 0, stream, patch, pos, B,
                       Np, D, x);
    return launch_status();
}

template <typename PatchT>
inline int pos_tokens_bwd_launch(const float* dx, int B, int Np, int D, PatchT* dpatch, float* dpos, hipStream_t stream) {
    LP_REQUIRE(dx && dpatch && dpos && B > 0 && Np > 0 && D > 0);
    if (D % 8 != 0) return LP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vit_pos_tokens_bwd_kernel<PatchT>, dim3(win_grid((long long)Np * (D / 8), 256)), dim3(256), 0, stream, dx, B, Np, D,
                       dpatch, dpos);
    return launch_status();
}

template <typename ElemT>
inline int resid_out_fwd_launch(const float* x, const ElemT* delta, size_t n, float* x_out, unsigned short* y, hipStream_t stream) {
    LP_REQUIRE(x && delta && x_out && n > 0);
    if (n % 8 != 0) return LP_ERR_UNSUPPORTED;
    const int blocks = win_grid((long long)(n / 8), 256);
    if (y != nullptr) hipLaunchKernelGGL((resid_out_fwd_kernel<ElemT, true>), dim3(blocks), dim3(256), 0, stream, x, delta, n / 8, x_out, y);
    else hipLaunchKernelGGL((resid_out_fwd_kernel<ElemT, false>), dim3(blocks), dim3(256), 0, stream, x, delta, n / 8, x_out, y);
    return launch_status();
}

template <typename ElemT>
inline int resid_out_bwd_launch(const ElemT* dy, size_t n, float* dx, hipStream_t stream) {
    LP_REQUIRE(dy && dx && n > 0);
    if (n % 8 != 0) return LP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(resid_out_bwd_kernel<ElemT>, dim3(win_grid((long long)(n / 8), 256)), dim3(256), 0, stream, dy, n / 8, dx);
    return launch_status();
}

}  // namespace lp

extern "C" int lp_window_partition(const void* src_bf16, int ld_src, int B, int gh, int gw, int ws, int cols, const void* fill_bf16,
                                   void* dst_bf16, lp_stream_t stream) {
    return lp::window_partition_launch((const unsigned short*)src_bf16, ld_src, B, gh, gw, ws, cols, (const unsigned short*)fill_bf16,
                                       (unsigned short*)dst_bf16, (hipStream_t)stream);
}

extern "C" int lp_window_unpartition(const void* src_bf16, int B, int gh, int gw, int ws, int cols, void* dst_bf16, int ld_dst,
                                     float* pad_colsum_acc, lp_stream_t stream) {
    return lp::window_unpartition_launch((const unsigned short*)src_bf16, B, gh, gw, ws, cols, (unsigned short*)dst_bf16, ld_dst, pad_colsum_acc,
                                         (hipStream_t)stream);
}

extern "C" int lp_f32_window_partition(const float* src, int ld_src, int B, int gh, int gw, int ws, int cols, const float* fill, float* dst,
                                       lp_stream_t stream) {
    return lp::window_partition_launch(src, ld_src, B, gh, gw, ws, cols, fill, dst, (hipStream_t)stream);
}

extern "C" int lp_f32_window_unpartition(const float* src, int B, int gh, int gw, int ws, int cols, float* dst, int ld_dst, float* pad_colsum_acc,
                                         lp_stream_t stream) {
    return lp::window_unpartition_launch(src, B, gh, gw, ws, cols, dst, ld_dst, pad_colsum_acc, (hipStream_t)stream);
}

extern "C" int lp_vit_pos_tokens_fwd(const void* patch_bf16, const float* pos, int B, int Np, int D, float* x, lp_stream_t stream) {
    return lp::pos_tokens_fwd_launch((const unsigned short*)patch_bf16, pos, B, Np, D, x, (hipStream_t)stream);
}

extern "C" int lp_vit_pos_tokens_bwd(const float* dx, int B, int Np, int D, void* dpatch_bf16, float* dpos, lp_stream_t stream) {
    return lp::pos_tokens_bwd_launch(dx, B, Np, D, (unsigned short*)dpatch_bf16, dpos, (hipStream_t)stream);
}

extern "C" int lp_f32_vit_pos_tokens_fwd(const float* patch, const float* pos, int B, int Np, int D, float* x, lp_stream_t stream) {
    return lp::pos_tokens_fwd_launch(patch, pos, B, Np, D, x, (hipStream_t)stream);
}

extern "C" int lp_f32_vit_pos_tokens_bwd(const float* dx, int B, int Np, int D, float* dpatch, float* dpos, lp_stream_t stream) {
    return lp::pos_tokens_bwd_launch(dx, B, Np, D, dpatch, dpos, (hipStream_t)stream);
}

extern "C" int lp_resid_out_fwd(const float* x, const void* delta_bf16, size_t n, float* x_out, void* y_bf16, lp_stream_t stream) {
    LP_REQUIRE(y_bf16);
    return lp::resid_out_fwd_launch(x, (const unsigned short*)delta_bf16, n, x_out, (unsigned short*)y_bf16, (hipStream_t)stream);
}

extern "C" int lp_resid_out_bwd(const void* dy_bf16, size_t n, float* dx, lp_stream_t stream) {
    return lp::resid_out_bwd_launch((const unsigned short*)dy_bf16, n, dx, (hipStream_t)stream);
}

extern "C" int lp_f32_resid_out_fwd(const float* x, const float* delta, size_t n, float* x_out, lp_stream_t stream) {
    return lp::resid_out_fwd_launch(x, delta, n, x_out, nullptr, (hipStream_t)stream);
}

extern "C" int lp_f32_resid_out_bwd(const float* dy, size_t n, float* dx, lp_stream_t stream) {
    return lp::resid_out_bwd_launch(dy, n, dx, (hipStream_t)stream);
}

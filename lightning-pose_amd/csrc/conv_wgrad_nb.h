// Weight gradient of the 3x3 / stride 1 / pad 1 layers with the input staged ONCE for all nine filter taps.
//
// conv_wgrad_pipe_kernel (conv_pipe.h) carries the filter tap in the load address of its `a` operand: a 256-wide a-tile is four taps x 64
// channels of the SAME pixels, every pixel row of x travels L2 -> LDS nine times and dy once per a-tile (48 KB into LDS per 1024 MFMA
// cycles), and the 9 Ci columns are padded to a multiple of 256.  Here a workgroup owns one 64-channel block of ci, one BN-wide block of
// co and one slice of the contraction, and accumulates all nine taps of that block (9 x 64 x BN fp32 = 144 / 72 accumulator registers
// per lane) from operands that enter LDS once: 64 rows of x (8 KB) and 64 rows of dy (BN x 128 B) per K step of 9 x 4 x BN/16 MFMAs.
//
// The contraction runs over a padded raster with SHARED borders: position P = (b (H + 1) + y + 1) (W + 1) + x + 1.  Column 0 of a raster
// row is the left border of that image row AND the right border of the row above; raster row b (H + 1) is the top border of image b AND
// the bottom border of image b - 1.  Border positions hold zeros in both operands (load masks: the buffer range check returns zeros), so
//   dW[r][s] = sum over ALL positions P of  x[P + (r - 1) (W + 1) + (s - 1)] (x) dy[P]
// with no case analysis anywhere: a tap is a constant row offset, across row ends and across images, and a K step is 64 consecutive
// positions.  The price is the MFMAs spent on border positions: (H + 1) (W + 1) / (H W) = 1.02 (96 x 96) ... 1.17 (12 x 12).
//
//   workgroup  512 threads = 8 waves.  BN = 128: wave = (ci half, co quarter), all four 16-position k-slices of a step.  BN = 64: wave =
//              (ci half, co half, K half): waves 0 - 3 take k-slices 0 - 1 of every step, waves 4 - 7 slices 2 - 3, and the two halves
//              leave as two partial tiles (the ordered reduction adds them like two pixel slices)
//   dy         ring of three stages [64 positions][BN channels], the B image of conv_wgrad_pipe_kernel (same swizzle, same fragments)
//   x          circular window of 512 raster rows x 128 B (64 KB) + a second copy of rows 0 - 63 behind it, so that a fragment's rows
//              base .. base + 52 never wrap and the k-slice / pixel-quad offsets ride in the instruction's offset field: ONE address
//              per tap and K step.  Only the 64 new rows are loaded per step; the loader runs `lead` = 1 + (W + 1) / 64 chunks ahead
//              of dy (the taps reach W + 2 rows forward) and the halo below the slice's first position is fetched once, in the prologue.
//              Window capacity: chunks kt - lead .. kt + 2 + lead live at once = 2 lead + 3 <= 8, i.e. W <= 126 (host-checked).
//   swizzle    16-B chunk c of raster row R sits at position c ^ (((R >> 1) & 1) << 2), applied on the source address of the load.
//              A 32-lane service group of ds_read_b64_tr_b16 reads 4 CONSECUTIVE rows x 64 B; rows alternate bank halves by R & 1 and
//              64-B halves by (R >> 1) & 1, so the four pieces always cover the 64 banks once.  Because positions are linear, a tap only
//              moves R by a constant and the four rows stay consecutive: the tap-shifted reads are conflict-free for every tap, width
//              and image boundary (the HALO form's pixel-indexed rows needed a jump-aware key for that, conv_pipe.h).
//   waits      one counted vmcnt wait + one barrier per K step, as in conv_pipe.h; transposed reads are the asm form, fetched one
//              filter row (3 taps) ahead of the MFMAs with counted lgkmcnt waits.
// The slices' partial tiles go to the workspace in accumulator order; wgrad_nb_reduce_kernel adds them in a fixed order (bit-reproducible).
#pragma once

namespace lp {

constexpr int kNbWin = 512, kNbMirror = 64;   // raster rows of the circular x window; rows kept a second time behind it
constexpr int kNbWinB = (kNbWin + kNbMirror) * 128;

struct WgradNbGeom {
    int B, H, W, Ci, Co;
    int PT;     // raster positions: B (H + 1) (W + 1)
    int lead;   // chunks the x loader runs ahead of dy: 1 + (W + 1) / 64
};

template <int BN>
__global__ __launch_bounds__(512) void conv_wgrad_nb_kernel(const unsigned short* __restrict__ X, const unsigned short* __restrict__ DY,
                                                            unsigned x_bytes, unsigned dy_bytes, WgradNbGeom g, int tiles, int tiles_b,
                                                            int p_per_split, FastDiv div_wp, FastDiv div_hp, float* __restrict__ ws) {
    constexpr int NWQ = BN / 16;             // waves that share a k-slice: (ci half) x (32-wide co block)
    constexpr int KH = 8 / NWQ;              // K halves (BN = 64: 2)
    constexpr int NKK = (kBK / 16) / KH;     // k-slices per wave and K step
    constexpr int NLB = BN / 64;             // dy loads per thread and K step
    constexpr int kRowB = BN * 2, kStageB = kBK * kRowB;
    constexpr int NG = NKK * 3;              // fragment groups per K step: (k-slice, filter row)
    __shared__ __attribute__((aligned(16))) unsigned char smem[3 * kStageB + kNbWinB];
    unsigned char* const xwin = smem + 3 * kStageB;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave % NWQ, kh = wave / NWQ;
    const int mt = wq & 1, nt = wq >> 1;
    const int work = xcd_remap(blockIdx.x, gridDim.x);    // slice slow: an XCD owns whole slices (all tiles of a slice share its L2)
    const int slice = work / tiles, tile = work - slice * tiles;
    const int ci0 = (tile / tiles_b) * 64, b0 = (tile % tiles_b) * BN;
    const int p_begin = slice * p_per_split, p_end = min(g.PT, p_begin + p_per_split);   // (p_per_split is a multiple of 64)
    const int KT = (p_end - p_begin + kBK - 1) / kBK;
    const int Wp = g.W + 1, Hp = g.H + 1;
    const buf_rsrc rsrc_x = make_buf_rsrc(X, x_bytes), rsrc_dy = make_buf_rsrc(DY, dy_bytes);

    // raster position -> pixel row of the NHWC tensors, or -1 on a border / outside the batch
    auto pixel_of = [&](int P) -> int {
        const bool in = P >= 0 && P < g.PT;
        const int Pc = in ? P : 0;
        const int row = fdiv(Pc, div_wp), xp = Pc - row * Wp;
        const int b = fdiv(row, div_hp), yp = row - b * Hp;
        return (in && xp >= 1 && yp >= 1) ? (b * g.H + yp - 1) * g.W + xp - 1 : -1;
    };

    // ---- loader.  x: chunk c = raster rows p_begin + 64 c .. + 63, wave w its rows 8 w .. 8 w + 7 (one instruction, 8 rows x 128 B).
    // dy (BN = 128): rows q * 32 + wave * 4 + (lane >> 4) (four 256-B rows); dy (BN = 64): rows wave * 8 + (lane >> 3)
    const int xrow = wave * 8 + (lane >> 3);
    auto load_x = [&](int c) {
        const int R0 = p_begin + c * kBK, R = R0 + xrow;
        const int m = c < KT + g.lead ? pixel_of(R) : -1;
        const int chunk = (lane & 7) ^ (((R >> 1) & 1) << 2);
        const unsigned voff = m >= 0 ? (unsigned)m * (unsigned)(g.Ci * 2) + (unsigned)(ci0 + chunk * 8) * 2u : ~0u;
        const int slot0 = R0 & (kNbWin - 1);
        buf_load16_lds(rsrc_x, xwin + (slot0 + wave * 8) * 128, voff, 0u);
        if (slot0 == 0) buf_load16_lds(rsrc_x, xwin + (kNbWin + wave * 8) * 128, voff, 0u);   // (wave-uniform) the copy behind the window
    };
    const int brow = (BN == 128) ? wave * 4 + (lane >> 4) : wave * 8 + (lane >> 3);   // + 32 q
    const int bchunk = (BN == 128) ? ((lane & 15) ^ ((brow & 3) << 2)) : ((lane & 7) ^ (((brow >> 1) & 1) << 2));
    const unsigned boff = (unsigned)(b0 + bchunk * 8) * 2u;
    unsigned is_b[NLB];
    unsigned char* is_dst = smem;
    auto prep_dy = [&](int st, int kt) {
#pragma unroll
        for (int q = 0; q < NLB; ++q) {
            const int P = p_begin + kt * kBK + q * 32 + brow;
            const int m = (P < p_end && kt < KT) ? pixel_of(P) : -1;
            is_b[q] = m >= 0 ? (unsigned)m * (unsigned)(g.Co * 2) + boff : ~0u;
        }
        is_dst = smem + st * kStageB;
    };
    auto issue_dy = [&]() {
#pragma unroll
        for (int q = 0; q < NLB; ++q) {
            if (BN == 128) buf_load16_lds(rsrc_dy, is_dst + (q * 32 + wave * 4) * kRowB, is_b[q], 0u);
            else buf_load16_lds(rsrc_dy, is_dst + (wave * 8) * kRowB, is_b[0], 0u);
        }
    };

    // ---- fragments (lp_common.h: lds_read_tr16): lane of 16-lane group fq supplies position 8 (fq / 2) + (fi / 4) of the k-slice (+ 4 for
    // the second read) and channels 16 (fq % 2) + 4 (fi % 4) .. + 3 of a 32-channel block; it receives channel lane % 32, positions 8 (lane / 32) .. + 7
    const int fq = lane >> 4, fi = lane & 15;
    const int frow = (fq >> 1) * 8 + (fi >> 2), fcol = (fq & 1) * 16 + (fi & 3) * 4;
    const int xe0 = mt * 32 + fcol;
    const int xrow0 = frow + kh * (NKK * 16);   // this lane's first row of a step, relative to the step's first position + the tap offset
    const int be0 = nt * 32 + fcol;
    const int swb = (BN == 128) ? ((frow & 3) << 2) : (((frow >> 1) & 1) << 2);
    const unsigned fob = (unsigned)((kh * (NKK * 16) + frow) * kRowB + (((be0 >> 3) ^ swb) << 4) + (be0 & 7) * 2);

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    const unsigned char* xa[9];   // per K step: this lane's address of tap t (k-slice and pixel quad are instruction offsets)
    int ld_kt = 2;                // the K step whose operands the next issue fetches
    auto mma_step = [&](int st) {
        const unsigned char* pb = smem + st * kStageB + fob;
        bf16x8 a[2][3], b[2];
        typedef __attribute__((ext_vector_type(8))) short s16x8_t;
        auto fetch = [&](auto gi_c) {
            constexpr int gi = decltype(gi_c)::value, kkl = gi / 3, r = gi % 3;
            if constexpr (r == 0) {
                const s16x4_t lo = lds_read_tr16_async_off<kkl * 16 * kRowB>(pb), hi = lds_read_tr16_async_off<kkl * 16 * kRowB + 4 * kRowB>(pb);
                const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                b[kkl & 1] = __builtin_bit_cast(bf16x8, v);
            }
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const s16x4_t lo = lds_read_tr16_async_off<kkl * 16 * 128>(xa[r * 3 + s]), hi = lds_read_tr16_async_off<kkl * 16 * 128 + 4 * 128>(xa[r * 3 + s]);
                const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                a[gi & 1][s] = __builtin_bit_cast(bf16x8, v);
            }
        };
        // group gi's reads must have returned before its MFMAs; group gi + 1's (6, or 8 with a new dy fragment) may still be in flight
        auto group = [&](auto gi_c) {
            constexpr int gi = decltype(gi_c)::value, kkl = gi / 3, r = gi % 3, set = gi & 1;
            if constexpr (gi + 1 < NG) fetch(std::integral_constant<int, gi + 1>{});
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (gi + 1 == NG) LP_WAIT_LGKM_TOUCH4(0, a[set][0], a[set][1], a[set][2], b[kkl & 1]);
            else if constexpr ((gi + 1) % 3 == 0) LP_WAIT_LGKM_TOUCH4(8, a[set][0], a[set][1], a[set][2], b[kkl & 1]);
            else LP_WAIT_LGKM_TOUCH4(6, a[set][0], a[set][1], a[set][2], b[kkl & 1]);
#pragma unroll
            for (int s = 0; s < 3; ++s) acc[r * 3 + s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[set][s], b[kkl & 1], acc[r * 3 + s], 0, 0, 0);
            if constexpr (gi == 0) {   // the next-but-one step's operands, behind the first MFMAs
                load_x(ld_kt + g.lead);
                issue_dy();
                ++ld_kt;
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        auto groups = [&](auto self, auto gi_c) {
            constexpr int gi = decltype(gi_c)::value;
            if constexpr (gi < NG) {
                group(gi_c);
                self(self, std::integral_constant<int, gi + 1>{});
            }
        };
        fetch(std::integral_constant<int, 0>{});
        groups(groups, std::integral_constant<int, 0>{});
    };

    // ---- prologue: the halo below the slice and the chunks of steps 0 and 1
    for (int c = -g.lead; c <= g.lead; ++c) load_x(c);
    prep_dy(0, 0);
    issue_dy();
    load_x(g.lead + 1);
    prep_dy(1, 1);
    issue_dy();
    int cur = 0;
    for (int kt = 0; kt < KT; ++kt) {
        // this wave's loads of step kt have landed; the x chunk and the NLB dy pieces of step kt + 1 stay in flight (a copy behind the
        // window is an extra load in some steps: the count is then conservative)
        if (NLB == 2) LP_WAIT_VM(3);
        else LP_WAIT_VM(2);
        LP_RAW_BARRIER();   // ... everyone's have, and everyone is done reading what the loads issued next overwrite
        const int R0 = p_begin + kt * kBK - Wp - 1 + xrow0;   // tap (0, 0)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int R = R0 + r * Wp + s;
                xa[r * 3 + s] = xwin + (((R & (kNbWin - 1)) << 7) | ((((xe0 >> 3) ^ ((R & 2) << 1))) << 4) | ((xe0 & 7) * 2));
            }
        prep_dy(cur == 0 ? 2 : cur - 1, kt + 2);   // (steps past the slice fetch nothing: the ring keeps its count)
        mma_step(cur);
        cur = cur == 2 ? 0 : cur + 1;
    }
    LP_WAIT_VM(0);
    // partial tile -> workspace[slice][K half][tile][wq][tap][e][lane] (accumulator order: every store is a full 256-B line per wave)
    float* dst = ws + ((((size_t)(slice * KH + kh) * tiles + tile) * NWQ + wq) * (9 * 16)) * 64 + lane;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) dst[(t * 16 + e) * 64] = acc[t][e];
}

// dW[co][tap][ci] += sum over (slice, K half) of the partial tiles, in order (deterministic).  One workgroup per 64 consecutive
// accumulator elements of a tile; its 4 waves stride over the partial tiles and combine through LDS (as wgrad_pipe_reduce_kernel).
template <int BN>
__global__ __launch_bounds__(256) void wgrad_nb_reduce_kernel(const float* __restrict__ ws, int parts, int tiles, int tiles_b, int Ci,
                                                              float* __restrict__ dW) {
    constexpr int NWQ = BN / 16;
    constexpr int PER_TILE = NWQ * 9 * 16 * 64;
    __shared__ float part[4][64];
    const size_t total = (size_t)tiles * PER_TILE;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + lane;
    float s0 = 0.f, s1 = 0.f;
    int sl = w;
    for (; sl + 4 < parts; sl += 8) {
        s0 += ws[(size_t)sl * total + i];
        s1 += ws[(size_t)(sl + 4) * total + i];
    }
    for (; sl < parts; sl += 4) s0 += ws[(size_t)sl * total + i];
    part[w][lane] = s0 + s1;
    __syncthreads();
    if (w == 0) {
        const float sum = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        size_t t = i >> 6;
        const int e = (int)(t & 15);
        t >>= 4;
        const int tap = (int)(t % 9);
        t /= 9;
        const int wq = (int)(t % NWQ);
        const int tile = (int)(t / NWQ);
        const int ci = (tile / tiles_b) * 64 + (wq & 1) * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        const int co = (tile % tiles_b) * BN + (wq >> 1) * 32 + (lane & 31);
        dW[((size_t)co * 9 + tap) * Ci + ci] += sum;
    }
}

}  // namespace lp

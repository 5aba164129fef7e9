// Prediction metrics over a device-resident table of keypoints: pixel error against labels, temporal norm, and the PCA reprojection error
// (single- and multi-view) per frame and keypoint.  gfx950, fp32, ONE launch, nothing read back.
//
// Reference arithmetic (paths relative to the reference tree):
//   metrics.py:47-59     pixel_error                          ||labels - pred||
//   metrics.py:62-89     temporal_norm (losses/losses.py:651-672 compute_loss): row 0 NaN, no epsilon, no confidence mask, no relu
//   metrics.py:92-184    pca_{single,multi}view_reprojection_error ; utils/pca.py:266-309 (reproject, compute_reprojection_error)
//
// Unlike the loss kernels of kploss.hip (one workgroup, a scalar out, relu(. - eps) folded in) the grid scales with T - an hour of 100 Hz
// video is 360 000 rows - and every output is a full (T, K) table.  A workgroup takes chunks of kMetFrames frames:
//   phase 1  pixel error and temporal norm, one thread per (frame, keypoint), flat and coalesced;
//   phase 2  the PCA tables in pca_kernel's form - one lane per point (P <= 64), the kept eigenvectors staged in LDS once per workgroup, a
//            projection coefficient = one reduction across lanes - with a wave holding as many samples as fit: a sample takes a group of
//            G = 2^ceil(log2 P) lanes (32 samples per wave for two views, 4 for 13 keypoints), the reduction runs over the group only.
// Every output element has exactly ONE writer, the NaN fills included: LDS holds per table an owner map column -> (position in the index
// table | -1), built once per workgroup; a lane stores its point's norm only if it owns the column (a column listed twice goes to its LAST
// entry, as numpy's fancy assignment does), and the columns nobody owns are filled by the workgroup that has the frame.  No memset beforehand, no
// atomics on global memory, no scratch: two runs, or two launch geometries, give the same bits.
// The residual is (x - mu) - V^T V (x - mu): the mean is never added back (the reference's form loses digits at frame scale).  Products and
// sums are NOT contracted into FMAs here, so the host build of this file (tests/hipemu) computes the same bits as the device.
// A NaN coordinate in a PCA sample reaches every coefficient through the wave sum, hence every entry of that sample, as in the reference's
// matmul.
#include "lp_common.h"

namespace lp {

constexpr int kMetWaves = 4;      // waves per workgroup
constexpr int kMetFrames = 64;    // frames per chunk
constexpr int kMetMaxGrid = 2048; // 8 workgroups per CU: a longer table walks its chunks with a grid stride
constexpr int kMetMaxPoints = 64; // one lane per point
constexpr size_t kMetMaxLds = 160 * 1024;

struct MetPca {            // one PCA table of the launch (out == nullptr: not wanted)
    const int* idx;        // (rows, P)
    const float* mean;     // (2 P)
    const float* ev;       // (ncomp, 2 P)
    float* out;            // (T, K)
    int rows, P, ncomp;
    int lg;                // a sample's lane group is 2^lg >= P lanes
};

// sum over each group of G consecutive lanes (G a power of two), every lane of the group gets it: the last log2 G steps of wave_sum
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float group_sum(float v, int lg) {   // (lg wave-uniform)
    switch (lg) {
        case 0: return v;
        case 1: return group_sum<2>(v);
        case 2: return group_sum<4>(v);
        case 3: return group_sum<8>(v);
        case 4: return group_sum<16>(v);
        case 5: return group_sum<32>(v);
        default: return group_sum<64>(v);
    }
}

// one table over the nf frames from f0; `ev` and `own` are this table's LDS images.  A sample takes a GROUP of G = 2^lg >= P lanes, one lane per
// point, so a wave holds 64 / G samples at a time (32 for two views) and a coefficient is a reduction over the group only.  The lanes of a
// group beyond P hold zeros: the sums are those of the whole-wave form, bit for bit.
__device__ __forceinline__ void met_pca_chunk(const float* __restrict__ pred, int K, const MetPca& p, const float* ev, const int* own, int f0,
                                              int nf, int tid) {
#pragma clang fp contract(off)
    const float nan = __int_as_float(0x7fc00000);
    const int lane = tid & 63, wave = tid >> 6;
    const int D = 2 * p.P, per = 64 >> p.lg, grp = lane >> p.lg, pt = lane & ((1 << p.lg) - 1);
    const bool has_pt = pt < p.P;
    const int lp = has_pt ? pt : 0;
    const float m0 = p.mean[2 * lp], m1 = p.mean[2 * lp + 1];
    const int n = nf * p.rows;   // samples of the chunk (nf <= 64, rows <= 2^24)
    for (int s0 = wave * per; s0 < n; s0 += kMetWaves * per) {   // (wave-uniform trip counts: the reductions involve every lane)
        const int s = s0 + grp;
        const bool act = has_pt && s < n;
        const int sc = s < n ? s : 0;   // (a group past the end computes on sample 0 and stores nothing)
        const int fl = sc / p.rows, j = sc - fl * p.rows;
        const int slot = j * p.P + lp;
        const int kk = p.idx[slot];
        const bool inb = (unsigned)kk < (unsigned)K;   // (the host refused such a table; a device copy that differs must not fault)
        const size_t row = (size_t)(f0 + fl) * K;
        const size_t e = (row + (size_t)(inb ? kk : 0)) * 2;
        const float x0 = !act ? 0.f : inb ? pred[e] - m0 : nan, x1 = !act ? 0.f : inb ? pred[e + 1] - m1 : nan;
        float r0 = x0, r1 = x1;
        for (int c = 0; c < p.ncomp; ++c) {
            const float e0 = act ? ev[c * D + 2 * lp] : 0.f, e1 = act ? ev[c * D + 2 * lp + 1] : 0.f;
            const float dot = group_sum(x0 * e0 + x1 * e1, p.lg);
            r0 = r0 - dot * e0;
            r1 = r1 - dot * e1;
        }
        if (act && inb && own[kk] == slot) p.out[row + kk] = sqrtf(r0 * r0 + r1 * r1);
    }
    const size_t base = (size_t)f0 * K;
    for (int e = tid; e < nf * K; e += 64 * kMetWaves)   // the columns nobody owns, flat over the chunk
        if (own[e % K] < 0) p.out[base + e] = nan;
}

__global__ __launch_bounds__(64 * kMetWaves) void kp_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ labels, int T, int K,
                                                                    MetPca sv, MetPca mv, float* __restrict__ pix, float* __restrict__ tmp,
                                                                    int n_chunks) {
#pragma clang fp contract(off)
    HIP_DYNAMIC_SHARED(float, smem)   // [sv.ncomp][2 sv.P] | [mv.ncomp][2 mv.P] | own_sv[K] | own_mv[K]   (a table that is not wanted takes nothing)
    const int tid = threadIdx.x;
    const int n_sv = sv.out ? sv.ncomp * 2 * sv.P : 0, n_mv = mv.out ? mv.ncomp * 2 * mv.P : 0;
    float* ev_sv = smem;
    float* ev_mv = smem + n_sv;
    int* own_sv = reinterpret_cast<int*>(smem + n_sv + n_mv);
    int* own_mv = own_sv + (sv.out ? K : 0);
    for (int i = tid; i < n_sv; i += 64 * kMetWaves) ev_sv[i] = sv.ev[i];
    for (int i = tid; i < n_mv; i += 64 * kMetWaves) ev_mv[i] = mv.ev[i];
    if (sv.out)
        for (int i = tid; i < K; i += 64 * kMetWaves) own_sv[i] = -1;
    if (mv.out)
        for (int i = tid; i < K; i += 64 * kMetWaves) own_mv[i] = -1;
    __syncthreads();
    if (sv.out)
        for (int i = tid; i < sv.rows * sv.P; i += 64 * kMetWaves) {
            const int kk = sv.idx[i];
            if ((unsigned)kk < (unsigned)K) atomicMax(&own_sv[kk], i);   // (LDS; the largest position wins whatever the order)
        }
    if (mv.out)
        for (int i = tid; i < mv.rows * mv.P; i += 64 * kMetWaves) {
            const int kk = mv.idx[i];
            if ((unsigned)kk < (unsigned)K) atomicMax(&own_mv[kk], i);
        }
    __syncthreads();

    const float nan = __int_as_float(0x7fc00000);
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int f0 = chunk * kMetFrames, f1 = f0 + kMetFrames < T ? f0 + kMetFrames : T;   // (T < 2^30: the launcher refuses 2 T K >= 2^31)
        if (pix || tmp) {
            const size_t e1 = (size_t)f1 * K;
            for (size_t e = (size_t)f0 * K + tid; e < e1; e += 64 * kMetWaves) {
                const float px = pred[2 * e], py = pred[2 * e + 1];
                if (pix) {
                    const float dx = labels[2 * e] - px, dy = labels[2 * e + 1] - py;
                    pix[e] = sqrtf(dx * dx + dy * dy);
                }
                if (tmp) {
                    float v = nan;
                    if (e >= (size_t)K) {   // frame >= 1
                        const float dx = px - pred[2 * (e - K)], dy = py - pred[2 * (e - K) + 1];
                        v = sqrtf(dx * dx + dy * dy);
                    }
                    tmp[e] = v;
                }
            }
        }
        if (sv.out) met_pca_chunk(pred, K, sv, ev_sv, own_sv, f0, f1 - f0, tid);
        if (mv.out) met_pca_chunk(pred, K, mv, ev_mv, own_mv, f0, f1 - f0, tid);
    }
}

static int met_log2_group(int points) {
    int lg = 0;
    while ((1 << lg) < points) ++lg;
    return lg;
}

// LP_OK, or why the table is refused; nothing here touches device memory
static int met_check_spec(const lp_pca_spec* s, int K, int single) {
    LP_REQUIRE(s->index && s->index_host && s->mean && s->rows > 0 && s->points > 0 && s->ncomp >= 0);
    LP_REQUIRE(s->points <= kMetMaxPoints && s->ncomp <= 2 * s->points);
    LP_REQUIRE(s->ncomp == 0 || s->kept_eigenvectors);
    LP_REQUIRE(!single || s->rows == 1);
    LP_REQUIRE((long long)s->rows * s->points <= (1 << 24));   // (sample counts of a chunk stay far inside 32 bits)
    for (long long i = 0; i < (long long)s->rows * s->points; ++i) LP_REQUIRE(s->index_host[i] >= 0 && s->index_host[i] < K);
    return LP_OK;
}

}  // namespace lp

extern "C" int lp_kp_metrics(const float* pred, const float* labels, int T, int K, const lp_pca_spec* singleview, const lp_pca_spec* multiview,
                             float* pixel_error, float* temporal_norm, float* pca_singleview, float* pca_multiview, lp_stream_t stream) {
    using namespace lp;
    LP_REQUIRE(pred && T > 0 && K > 0);
    LP_REQUIRE(pixel_error || temporal_norm || pca_singleview || pca_multiview);
    LP_REQUIRE(!pixel_error || labels);
    LP_REQUIRE(!pca_singleview || singleview);
    LP_REQUIRE(!pca_multiview || multiview);
    MetPca sv{}, mv{};
    size_t smem = 0;
    if (pca_singleview) {
        const int rc = met_check_spec(singleview, K, 1);
        if (rc != LP_OK) return rc;
        sv = MetPca{singleview->index, singleview->mean, singleview->kept_eigenvectors, pca_singleview, 1, singleview->points, singleview->ncomp,
                    met_log2_group(singleview->points)};
        smem += ((size_t)sv.ncomp * 2 * sv.P + (size_t)K) * 4;
    }
    if (pca_multiview) {
        const int rc = met_check_spec(multiview, K, 0);
        if (rc != LP_OK) return rc;
        mv = MetPca{multiview->index, multiview->mean, multiview->kept_eigenvectors, pca_multiview, multiview->rows, multiview->points,
                    multiview->ncomp, met_log2_group(multiview->points)};
        smem += ((size_t)mv.ncomp * 2 * mv.P + (size_t)K) * 4;
    }
    if (2ll * T * K >= (1ll << 31)) return LP_ERR_UNSUPPORTED;   // (the offsets are 64-bit; tables this large have never been run)
    if (smem > kMetMaxLds) return LP_ERR_UNSUPPORTED;            // the eigenvectors and owner maps of both tables must fit one workgroup's LDS
    if (smem > 32 * 1024)   // (opt in to a large dynamic LDS window; gfx950 has 160 KB per workgroup)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kp_metrics_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    const int n_chunks = (int)(((long long)T + kMetFrames - 1) / kMetFrames);
    const int grid = n_chunks < kMetMaxGrid ? n_chunks : kMetMaxGrid;
    hipLaunchKernelGGL(kp_metrics_kernel, dim3(grid), dim3(64 * kMetWaves), smem, (hipStream_t)stream, pred, labels, T, K, sv, mv, pixel_error,
                       temporal_norm, n_chunks);
    return launch_status();
}

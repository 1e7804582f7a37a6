// glp_kernels.hip -- the LPIPS evaluation metric (include/glp.h): lpipsPyTorch's forward for the alex and vgg backbones on kernels of our own,
// so that neither torchvision nor a download is needed (the weights are files the user hands over: gaussianavatars_amd/lpips.py).
//
// k_conv is the whole cost: a direct convolution as an implicit GEMM, D[cout][pixel] = sum_kk W[cout][kk] * im2col[kk][pixel] with
// kk = (c*k + ky)*k + kx, on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate, exact: bf16 would change the metric).  A workgroup of four waves
// owns 64 output channels x 64 output pixels; wave w owns channels 16w..16w+15 of all 64 pixels, four 16x16 tiles.  The reduction runs in blocks
// of 16: the weights' block comes from the K-major packed copy (coalesced, zero-padded past K, so the K tail -- 27, 363 -- needs no test on that
// side) and the im2col block is gathered from x into LDS and never exists in memory; a position outside the image, past K or past the last
// pixel gathers 0.  The next block's global loads are issued before the current block's MFMAs.  The four k-steps of a block accumulate into four
// SEPARATE accumulators that are added pairwise at the end: four independent MFMA chains per tile, and a fmaf chain of K/4 instead of K terms
// (fp32 summation error grows with the length of the chain).  Bias and ReLU are applied to the accumulators on their way out.
// k_head reads a tap's features of both images, k_finish adds the five taps: fixed order, fp64 partials, no atomics.
// Built with -ffp-contract=fast: nothing here is compared bit for bit against a host (the pool moves values, it computes none).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/glp.h"
#include "launch_prof.h"
#include "lib_common.h"
#include "wave_reduce.h"

namespace glp {

using wave_reduce::wave_sum_hi;   // sum over the 64 lanes, valid in lane 63
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = GLP_TILE, BN = GLP_TILE, BK = GLP_KBLOCK;
constexpr int LDS_ROW = 80;   // floats per LDS row: 64 + 16, so that the four k rows one MFMA operand load touches fall into four different groups of 16 banks
static_assert(BM == 64 && BN == 64 && BK == 16, "the thread roles below are written for 64 x 64 x 16 and 256 threads");

// what one thread brings in per reduction block: rows kr0, kr0 + 4, kr0 + 8, kr0 + 12 of column `col` of both operands
template <int KS>
__device__ __forceinline__ void fetch(float (&ra)[4], float (&rb)[4], int k0, int kr0, const float* __restrict__ wcol, int Cout,
                                      const float* __restrict__ ximg, bool pix_ok, int K, int H, int W, int iy0, int ix0)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kk = k0 + kr0 + 4 * i;
        ra[i] = wcol[(size_t)kk * Cout];   // (kk < the padded K: the packed copy has that row, zeros past K)
        float v = 0.f;
        if (pix_ok && kk < K) {
            const int c = kk / (KS * KS), r = kk - c * (KS * KS), ky = r / KS, kx = r - ky * KS;
            const int iy = iy0 + ky, ix = ix0 + kx;
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = ximg[((size_t)c * H + iy) * W + ix];
        }
        rb[i] = v;
    }
}

template <int KS>
__global__ __launch_bounds__(256) void k_conv(int Cin, int H, int W, int Cout, int stride, int pad, int Ho, int Wo, int npix, int K, int Kpad,
                                               const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias, int relu,
                                               float* __restrict__ out)
{
    __shared__ float As[BK][LDS_ROW], Bs[BK][LDS_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int howo = Ho * Wo;
    // loading role: column `col` (an output channel of the weights' block, an output pixel of the gather's), rows kr0 + 4i
    const int col = tid & 63, kr0 = tid >> 6;
    const int p = n0 + col;
    const bool pix_ok = p < npix;
    const int img = pix_ok ? p / howo : 0, rem = p - img * howo, oy = rem / Wo, ox = rem - oy * Wo;
    const int iy0 = oy * stride - pad, ix0 = ox * stride - pad;
    const float* __restrict__ ximg = x + (size_t)img * Cin * H * W;
    const float* __restrict__ wcol = wp + m0 + col;

    f32x4 acc[4][4];   // [k-step of the block][pixel tile]
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[s][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float ra[4], rb[4];
    fetch<KS>(ra, rb, 0, kr0, wcol, Cout, ximg, pix_ok, K, H, W, iy0, ix0);
    const int arow = lane >> 4, acol = lane & 15;   // operand maps of 16x16x4: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
    for (int k0 = 0; k0 < Kpad; k0 += BK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[kr0 + 4 * i][col] = ra[i];
            Bs[kr0 + 4 * i][col] = rb[i];
        }
        __syncthreads();
        if (k0 + BK < Kpad) fetch<KS>(ra, rb, k0 + BK, kr0, wcol, Cout, ximg, pix_ok, K, H, W, iy0, ix0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float a = As[4 * s + arow][16 * wave + acol];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[s][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[4 * s + arow][16 * j + acol], acc[s][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: column (pixel) = lane & 15, row (channel) = 4 * (lane >> 4) + register
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = n0 + 16 * j + acol;
        if (q >= npix) continue;
        const int qi = q / howo, qr = q - qi * howo;
        const f32x4 sum = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = m0 + 16 * wave + 4 * arow + r;
            float v = sum[r] + (bias ? bias[co] : 0.f);
            if (relu) v = fmaxf(v, 0.f);
            out[((size_t)qi * Cout + co) * howo + qr] = v;
        }
    }
}

__global__ __launch_bounds__(256) void k_pack(int K, int Kpad, int Cout, const float* __restrict__ w, float* __restrict__ packed)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Kpad * Cout) return;
    const int kk = (int)(i / Cout), co = (int)(i - (long long)kk * Cout);
    packed[i] = kk < K ? w[(size_t)co * K + kk] : 0.f;
}

__global__ __launch_bounds__(256) void k_maxpool(long long total, int H, int W, int Ho, int Wo, int k, int stride, const float* __restrict__ x,
                                                  float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long t = i / Wo, plane = t / Ho;
    const int ox = (int)(i - t * Wo), oy = (int)(t - plane * Ho);
    const float* __restrict__ base = x + ((size_t)plane * H + (size_t)oy * stride) * W + (size_t)ox * stride;   // floor mode: the window is inside
    float m = base[0];
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const float v = base[(size_t)dy * W + dx];
            if (v > m || v != v) m = v;   // torch's rule: a NaN wins
        }
    out[i] = m;
}

__global__ __launch_bounds__(256) void k_zscore(long long total, int B, int HW, const float* __restrict__ x, const float* __restrict__ y,
                                                 float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long plane = i / HW;
    const int c = (int)(plane % 3);
    const long long half = (long long)B * 3 * HW;
    const float v = i < half ? x[i] : y[i - half];
    const float mean = c == 0 ? -.030f : c == 1 ? -.088f : -.188f;
    const float sd = c == 0 ? .458f : c == 1 ? .448f : .450f;
    out[i] = (v - mean) / sd;
}

// a thread takes pair b, position q (neighbouring lanes neighbouring positions), and walks the C channels of both images twice: the norms, then
// the weighted squared difference of the normalised features (the second walk finds the tile in cache; the difference is formed from the two
// quotients themselves, never expanded, so an identical pair is exactly 0)
__global__ __launch_bounds__(256) void k_head(int B, int C, int HW, const float* __restrict__ feat, const float* __restrict__ lin,
                                               double* __restrict__ partial)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const long long items = (long long)B * HW, step = (long long)gridDim.x * 256;
    double total = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < items; i += step) {
        const int b = (int)(i / HW), q = (int)(i - (long long)b * HW);
        const float* __restrict__ fx = feat + (size_t)b * C * HW + q;
        const float* __restrict__ fy = feat + (size_t)(B + b) * C * HW + q;
        float sx = 0.f, sy = 0.f;
        for (int c = 0; c < C; ++c) {
            const float a = fx[(size_t)c * HW], d = fy[(size_t)c * HW];
            sx += a * a;
            sy += d * d;
        }
        const float nx = sqrtf(sx) + 1e-10f, ny = sqrtf(sy) + 1e-10f;   // eps outside the root: an all-zero position divides 0 by 1e-10
        float s = 0.f;
        for (int c = 0; c < C; ++c) {
            const float d = fx[(size_t)c * HW] / nx - fy[(size_t)c * HW] / ny;
            s += lin[c] * (d * d);
        }
        total += (double)s;
    }
    total = wave_sum_hi(total);
    if ((tid & 63) == 63) red[tid >> 6] = total;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct Finish {
    int blocks[GLP_TAPS];
    int hw[GLP_TAPS];
};

__global__ __launch_bounds__(256) void k_finish(const double* __restrict__ partial, Finish f, float* __restrict__ out)
{
    __shared__ double red[GLP_TAPS][4];
    const int tid = threadIdx.x;
    for (int t = 0; t < GLP_TAPS; ++t) {
        double v = tid < f.blocks[t] ? partial[t * GLP_HEAD_BLOCKS + tid] : 0.0;   // blocks <= GLP_HEAD_BLOCKS == the workgroup
        v = wave_sum_hi(v);
        if ((tid & 63) == 63) red[t][tid >> 6] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    double sum = 0.0;
    for (int t = 0; t < GLP_TAPS; ++t) {
        const double term = ((red[t][0] + red[t][1]) + (red[t][2] + red[t][3])) / (double)f.hw[t];
        out[t] = (float)term;
        sum += term;
    }
    out[GLP_TAPS] = (float)sum;
}
static_assert(GLP_HEAD_BLOCKS == 256, "k_finish reads one partial per thread");

// ---- the two layer tables (torchvision's `features`, up to the last tap) -------------------------------------------------------------
struct Op {
    int pool;   // 0: convolution followed by ReLU, 1: max pool
    int cin, cout, k, stride, pad;
    int tap;    // the activation after this op's ReLU is tapped
};
static const Op ALEX[] = {
    {0, 3, 64, 11, 4, 2, 1},  {1, 0, 0, 3, 2, 0, 0},     {0, 64, 192, 5, 1, 2, 1},  {1, 0, 0, 3, 2, 0, 0},
    {0, 192, 384, 3, 1, 1, 1}, {0, 384, 256, 3, 1, 1, 1}, {0, 256, 256, 3, 1, 1, 1},
};
static const Op VGG[] = {
    {0, 3, 64, 3, 1, 1, 0},    {0, 64, 64, 3, 1, 1, 1},   {1, 0, 0, 2, 2, 0, 0},     {0, 64, 128, 3, 1, 1, 0},  {0, 128, 128, 3, 1, 1, 1},
    {1, 0, 0, 2, 2, 0, 0},     {0, 128, 256, 3, 1, 1, 0}, {0, 256, 256, 3, 1, 1, 0}, {0, 256, 256, 3, 1, 1, 1}, {1, 0, 0, 2, 2, 0, 0},
    {0, 256, 512, 3, 1, 1, 0}, {0, 512, 512, 3, 1, 1, 0}, {0, 512, 512, 3, 1, 1, 1}, {1, 0, 0, 2, 2, 0, 0},     {0, 512, 512, 3, 1, 1, 0},
    {0, 512, 512, 3, 1, 1, 0}, {0, 512, 512, 3, 1, 1, 1},
};

struct Step {
    Op op;
    int C, H, W;      // the input
    int Co, Ho, Wo;   // the output
};

}  // namespace glp

// ---------------------------------------------------------------------------------------------------------------
using glp::Op;
using glp::Step;

static bool out_size(int H, int W, int k, int stride, int pad, int* Ho, int* Wo)
{
    const int h = H + 2 * pad - k, w = W + 2 * pad - k;
    if (h < 0 || w < 0) return false;
    *Ho = h / stride + 1;
    *Wo = w / stride + 1;
    return true;
}

// the shapes of every layer of `net` on H x W images; false when the net is unknown or a layer would be empty
static bool plan(int32_t net, int32_t H, int32_t W, std::vector<Step>* steps)
{
    const Op* ops = net == GLP_NET_ALEX ? glp::ALEX : net == GLP_NET_VGG ? glp::VGG : nullptr;
    if (!ops) return false;
    const int n = net == GLP_NET_ALEX ? (int)(sizeof glp::ALEX / sizeof(Op)) : (int)(sizeof glp::VGG / sizeof(Op));
    int C = 3;
    for (int i = 0; i < n; ++i) {
        Step s{ops[i], C, H, W, ops[i].pool ? C : ops[i].cout, 0, 0};
        if (!out_size(H, W, s.op.k, s.op.stride, s.op.pad, &s.Ho, &s.Wo)) return false;
        steps->push_back(s);
        C = s.Co, H = s.Ho, W = s.Wo;
    }
    return true;
}

static bool conv_shape_ok(int32_t Cin, int32_t Cout, int32_t k) { return Cin >= 1 && Cout >= 1 && (k == 1 || k == 3 || k == 5 || k == 11); }
static int padded_k(int K) { return (K + GLP_KBLOCK - 1) / GLP_KBLOCK * GLP_KBLOCK; }

static int conv_impl(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t k, int32_t stride, int32_t pad, const float* x,
                     const float* packed, const float* bias, int32_t relu, float* out, hipStream_t stream)
{
    if (N < 1 || H < 1 || W < 1) return fail(GLP_E_ARG, "bad image shape (%d,%d,%d,%d)", N, Cin, H, W);
    if (!conv_shape_ok(Cin, Cout, k)) return fail(GLP_E_ARG, "bad kernel shape (Cout %d, Cin %d, k %d): k is 1, 3, 5 or 11", Cout, Cin, k);
    if (Cout % GLP_TILE) return fail(GLP_E_ARG, "Cout %d is not a multiple of %d", Cout, GLP_TILE);
    if (stride < 1 || pad < 0 || pad >= k) return fail(GLP_E_ARG, "bad stride %d or padding %d", stride, pad);
    int Ho, Wo;
    if (!out_size(H, W, k, stride, pad, &Ho, &Wo)) return fail(GLP_E_ARG, "image %dx%d is smaller than the %dx%d kernel", H, W, k, k);
    if (!x || !packed || !out) return fail(GLP_E_ARG, "null pointer");
    if (x == out) return fail(GLP_E_ARG, "out must not alias x");
    if (((uintptr_t)x | (uintptr_t)packed | (uintptr_t)bias | (uintptr_t)out) & 3) return fail(GLP_E_ARG, "float buffers must be 4-byte aligned");
    const int64_t npix = (int64_t)N * Ho * Wo, K = (int64_t)Cin * k * k;
    if (npix > INT32_MAX - GLP_TILE || K > (1 << 24) || (int64_t)Cin * H * W > INT32_MAX) return fail(GLP_E_ARG, "convolution too large");
    const dim3 grid((unsigned)((npix + GLP_TILE - 1) / GLP_TILE), (unsigned)(Cout / GLP_TILE));
#define GLP_CONV(KS)                                                                                                                       \
    PROF_LAUNCH(glp::k_conv<KS>, grid, dim3(256), 0, stream, (int)Cin, (int)H, (int)W, (int)Cout, (int)stride, (int)pad, Ho, Wo, (int)npix, \
                (int)K, padded_k((int)K), x, packed, bias, (int)relu, out)
    if (k == 1) GLP_CONV(1);
    else if (k == 3) GLP_CONV(3);
    else if (k == 5) GLP_CONV(5);
    else GLP_CONV(11);
#undef GLP_CONV
    LAUNCH_CHECK(GLP_E_HIP, "k_conv");
    return GLP_OK;
}

static int pool_impl(int64_t planes, int32_t H, int32_t W, int32_t k, int32_t stride, const float* x, float* out, hipStream_t stream)
{
    if (planes < 1 || H < 1 || W < 1) return fail(GLP_E_ARG, "bad plane shape (%lld,%d,%d)", (long long)planes, H, W);
    if (!((k == 3 || k == 2) && stride == 2)) return fail(GLP_E_ARG, "max pool is k3 s2 or k2 s2, got k%d s%d", k, stride);
    if (H < k || W < k) return fail(GLP_E_ARG, "image %dx%d is smaller than the %dx%d window", H, W, k, k);
    if (!x || !out) return fail(GLP_E_ARG, "null pointer");
    if (x == out) return fail(GLP_E_ARG, "out must not alias x");
    const int Ho = (H - k) / stride + 1, Wo = (W - k) / stride + 1;
    const int64_t total = planes * Ho * Wo;
    if (total > (int64_t)INT32_MAX * 256) return fail(GLP_E_ARG, "pool too large");
    PROF_LAUNCH(glp::k_maxpool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (long long)total, (int)H, (int)W, Ho, Wo, (int)k,
                (int)stride, x, out);
    LAUNCH_CHECK(GLP_E_HIP, "k_maxpool");
    return GLP_OK;
}

static int zscore_impl(int32_t B, int32_t H, int32_t W, const float* x, const float* y, float* out, hipStream_t stream)
{
    if (B < 1 || H < 1 || W < 1) return fail(GLP_E_ARG, "bad image shape (%d,3,%d,%d)", B, H, W);
    if (!x || !y || !out) return fail(GLP_E_ARG, "null pointer");
    const int64_t HW = (int64_t)H * W, total = 2 * (int64_t)B * 3 * HW;
    if (HW > INT32_MAX || total > (int64_t)INT32_MAX * 256) return fail(GLP_E_ARG, "image too large");
    PROF_LAUNCH(glp::k_zscore, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (long long)total, (int)B, (int)HW, x, y, out);
    LAUNCH_CHECK(GLP_E_HIP, "k_zscore");
    return GLP_OK;
}

static int32_t head_blocks(int64_t items)
{
    const int64_t n = (items + 255) / 256;
    return (int32_t)(n < GLP_HEAD_BLOCKS ? n : GLP_HEAD_BLOCKS);
}

static int head_impl(int32_t B, int32_t C, int32_t H, int32_t W, const float* feat, const float* lin, double* partial, hipStream_t stream)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(GLP_E_ARG, "bad feature shape (2*%d,%d,%d,%d)", B, C, H, W);
    if (!feat || !lin || !partial) return fail(GLP_E_ARG, "null pointer");
    if ((uintptr_t)partial & 7) return fail(GLP_E_ARG, "partial must be 8-byte aligned");
    const int64_t HW = (int64_t)H * W;
    if (HW > INT32_MAX || B * HW > INT32_MAX) return fail(GLP_E_ARG, "feature map too large");
    PROF_LAUNCH(glp::k_head, dim3((unsigned)head_blocks(B * HW)), dim3(256), 0, stream, (int)B, (int)C, (int)HW, feat, lin, partial);
    LAUNCH_CHECK(GLP_E_HIP, "k_head");
    return GLP_OK;
}

static int finish_impl(const double* partial, const int32_t* blocks, const int32_t* hw, float* out, hipStream_t stream)
{
    if (!partial || !blocks || !hw || !out) return fail(GLP_E_ARG, "null pointer");
    if ((uintptr_t)partial & 7) return fail(GLP_E_ARG, "partial must be 8-byte aligned");
    glp::Finish f;
    for (int t = 0; t < GLP_TAPS; ++t) {
        if (blocks[t] < 1 || blocks[t] > GLP_HEAD_BLOCKS || hw[t] < 1) return fail(GLP_E_ARG, "tap %d: bad block count %d or size %d", t, blocks[t], hw[t]);
        f.blocks[t] = blocks[t], f.hw[t] = hw[t];
    }
    PROF_LAUNCH(glp::k_finish, dim3(1), dim3(256), 0, stream, partial, f, out);
    LAUNCH_CHECK(GLP_E_HIP, "k_finish");
    return GLP_OK;
}

// floats of one activation buffer of the plan: the z-scored input or the largest layer output, for 2B images
static int64_t buffer_floats(const std::vector<Step>& steps, int32_t B, int32_t H, int32_t W)
{
    int64_t most = 3 * (int64_t)H * W;
    for (const Step& s : steps) {
        const int64_t n = (int64_t)s.Co * s.Ho * s.Wo;
        most = n > most ? n : most;
    }
    return (2 * (int64_t)B * most + 3) / 4 * 4;   // (a multiple of four floats: the second buffer and the partials stay 16-byte aligned)
}

extern "C" {

int glp_abi_version(void) { return GLP_ABI_VERSION; }
const char* glp_last_error(void) { return g_err; }

int glp_net_convs(int32_t net)
{
    if (net == GLP_NET_ALEX) return 5;
    if (net == GLP_NET_VGG) return GLP_MAX_CONVS;
    return fail(GLP_E_ARG, "unknown net %d", net);
}

int64_t glp_packed_floats(int32_t Cin, int32_t Cout, int32_t k)
{
    if (!conv_shape_ok(Cin, Cout, k)) return fail(GLP_E_ARG, "bad kernel shape (Cout %d, Cin %d, k %d): k is 1, 3, 5 or 11", Cout, Cin, k);
    const int64_t K = (int64_t)Cin * k * k;
    if (K > (1 << 24)) return fail(GLP_E_ARG, "convolution too large");
    return (int64_t)padded_k((int)K) * Cout;
}

int glp_pack_weights(int32_t Cin, int32_t Cout, int32_t k, const float* w, float* packed, void* stream)
{
    const int64_t n = glp_packed_floats(Cin, Cout, k);
    if (n < 0) return (int)n;
    if (!w || !packed) return fail(GLP_E_ARG, "null pointer");
    const int K = Cin * k * k;
    PROF_LAUNCH(glp::k_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, K, padded_k(K), (int)Cout, w, packed);
    LAUNCH_CHECK(GLP_E_HIP, "k_pack");
    return GLP_OK;
}

int glp_conv2d(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t k, int32_t stride, int32_t pad, const float* x,
               const float* packed, const float* bias, int32_t relu, float* out, void* stream)
{
    return conv_impl(N, Cin, H, W, Cout, k, stride, pad, x, packed, bias, relu, out, (hipStream_t)stream);
}

int glp_maxpool(int64_t planes, int32_t H, int32_t W, int32_t k, int32_t stride, const float* x, float* out, void* stream)
{
    return pool_impl(planes, H, W, k, stride, x, out, (hipStream_t)stream);
}

int glp_zscore(int32_t B, int32_t H, int32_t W, const float* x, const float* y, float* out, void* stream)
{
    return zscore_impl(B, H, W, x, y, out, (hipStream_t)stream);
}

int32_t glp_head_blocks(int32_t B, int32_t H, int32_t W)
{
    if (B < 1 || H < 1 || W < 1) return fail(GLP_E_ARG, "bad feature shape (2*%d,C,%d,%d)", B, H, W);
    return head_blocks((int64_t)B * H * W);
}

int glp_head(int32_t B, int32_t C, int32_t H, int32_t W, const float* feat, const float* lin, double* partial, void* stream)
{
    return head_impl(B, C, H, W, feat, lin, partial, (hipStream_t)stream);
}

int glp_finish(const double* partial, const int32_t* blocks, const int32_t* hw, float* out, void* stream)
{
    return finish_impl(partial, blocks, hw, out, (hipStream_t)stream);
}

int64_t glp_workspace_bytes(int32_t net, int32_t B, int32_t H, int32_t W)
{
    if (net != GLP_NET_ALEX && net != GLP_NET_VGG) return fail(GLP_E_ARG, "unknown net %d", net);
    if (B < 1 || H < 1 || W < 1) return fail(GLP_E_ARG, "bad image shape (%d,3,%d,%d)", B, H, W);
    std::vector<Step> steps;
    if (!plan(net, H, W, &steps)) return fail(GLP_E_ARG, "image %dx%d is too small for this net", H, W);
    return 2 * buffer_floats(steps, B, H, W) * (int64_t)sizeof(float) + GLP_TAPS * GLP_HEAD_BLOCKS * (int64_t)sizeof(double);
}

int glp_forward(int32_t net, int32_t B, int32_t H, int32_t W, const float* x, const float* y, const void* const* conv_w,
                const void* const* conv_b, const void* const* lin, void* workspace, float* out, void* stream_)
{
    const int64_t bytes = glp_workspace_bytes(net, B, H, W);
    if (bytes < 0) return (int)bytes;
    if (!x || !y || !conv_w || !conv_b || !lin || !workspace || !out) return fail(GLP_E_ARG, "null pointer");
    if ((uintptr_t)workspace & 15) return fail(GLP_E_ARG, "workspace must be 16-byte aligned");
    const int convs = glp_net_convs(net);
    for (int i = 0; i < convs; ++i)
        if (!conv_w[i] || !conv_b[i]) return fail(GLP_E_ARG, "convolution %d: null weights or bias", i);
    for (int t = 0; t < GLP_TAPS; ++t)
        if (!lin[t]) return fail(GLP_E_ARG, "tap %d: null weights", t);
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<Step> steps;
    plan(net, H, W, &steps);
    const int64_t nbuf = buffer_floats(steps, B, H, W);
    float* buf[2] = {(float*)workspace, (float*)workspace + nbuf};
    double* partial = (double*)((float*)workspace + 2 * nbuf);
    int rc = zscore_impl(B, H, W, x, y, buf[0], stream);
    if (rc) return rc;
    int cur = 0, conv = 0, tap = 0;
    int32_t blocks[GLP_TAPS], hw[GLP_TAPS];
    for (const Step& s : steps) {
        if (s.op.pool)
            rc = pool_impl(2 * (int64_t)B * s.C, s.H, s.W, s.op.k, s.op.stride, buf[cur], buf[cur ^ 1], stream);
        else {
            rc = conv_impl(2 * B, s.C, s.H, s.W, s.Co, s.op.k, s.op.stride, s.op.pad, buf[cur], (const float*)conv_w[conv], (const float*)conv_b[conv], 1,
                           buf[cur ^ 1], stream);
            ++conv;
        }
        if (rc) return rc;
        cur ^= 1;
        if (s.op.tap) {
            rc = head_impl(B, s.Co, s.Ho, s.Wo, buf[cur], (const float*)lin[tap], partial + tap * GLP_HEAD_BLOCKS, stream);
            if (rc) return rc;
            blocks[tap] = head_blocks((int64_t)B * s.Ho * s.Wo);
            hw[tap] = s.Ho * s.Wo;
            ++tap;
        }
    }
    return finish_impl(partial, blocks, hw, out, stream);
}

LPROF_EXPORTS(glp)

}  // extern "C"

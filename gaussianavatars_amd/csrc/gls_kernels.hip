// gls_kernels.hip -- fused L1 + SSIM image loss (forward / backward) and the densification statistics
// update: the training-step neighbours of the render path (include/gls.h).
//
// SSIM forward, per output tile: the five windowed moments E[x], E[y], E[x^2], E[y^2], E[xy] are formed by the
// separable window of ssim_window.h (halo to LDS, horizontal taps into LDS, vertical taps in registers), the
// SSIM map and |x-y| are reduced per workgroup into fixed-order partials, and the three partial derivatives
// the backward needs are written as planes.  Backward: the same window over those three planes, combined
// with x and y.  All of it is HBM-trivial (5 MB images); the point is ~4 launches instead of ~60.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "../../include/gls.h"
#include "launch_prof.h"
#include "lib_common.h"
#include "ssim_window.h"
#include "wave_reduce.h"

namespace gls {

// the tile scheme of the SSIM kernels (32 x 16 tiles, the halo, the register-blocked taps and what was measured) is ssim_window.h's
using namespace ssim_window;
using wave_reduce::wave_sum_hi;   // sum over the 64 lanes, valid in lane 63
static_assert(WIN == GLS_SSIM_WINDOW, "include/gls.h publishes the window ssim_window.h applies");

// the halo of one fp32 plane
__device__ __forceinline__ void load_halo(float (*dst)[HXS], const float* __restrict__ plane, int H, int W, int x0, int y0, int tid)
{
    ssim_window::load_halo(dst, H, W, x0, y0, tid, [=](int gy, int gx) { return plane[(size_t)gy * W + gx]; });
}

__global__ __launch_bounds__(256, 6) void k_l1_ssim_fwd(int H, int W, const float* __restrict__ img1, const float* __restrict__ img2,
                                                      Window win, float* __restrict__ maps, size_t map_stride,
                                                      float2* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float sx[HY][HXS], sy[HY][HXS];
    __shared__ __attribute__((aligned(16))) float hq[5][HY][TX];
    __shared__ float red[2][4];
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const size_t poff = (size_t)plane * H * W;
    load_halo(sx, img1 + poff, H, W, x0, y0, tid);
    load_halo(sy, img2 + poff, H, W, x0, y0, tid);
    __syncthreads();
    horizontal_pair(sx, sy, hq, win, tid);
    __syncthreads();
    const int tx = tid & 31, ty0 = (tid >> 5) * 2;   // vertical taps: column tx, rows ty0 and ty0 + 1
    float col[5][WIN + 1];
    load_columns(hq, tx, ty0, col);
    float l1 = 0.f, ss = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float e[5];   // E[x], E[y], E[x^2], E[y^2], E[xy]
        window_sums(col, win, j, e);
        const float mu1 = e[0], mu2 = e[1], e11 = e[2], e22 = e[3], e12 = e[4];
        const int ty = ty0 + j, px = x0 + tx, py = y0 + ty;
        if (px < W && py < H) {
            // (no contraction from here on, and the map as the product of two quotients: for an identical pair A == C and B == D bit for
            //  bit, so the map is exactly 1, d m / d mu1 exactly 0 and d m / d E[xy] exactly -2 d m / d E[x^2], and the backward returns the
            //  zero gradient the reference returns.  Contracted, 2 x cb + y cc left the rounding of one product behind: 1e-8 at one pixel.)
#pragma clang fp contract(off)
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
            const float A = 2.f * mu12 + SSIM_C1, Bv = 2.f * s12 + SSIM_C2;
            const float Cv = mu1_sq + mu2_sq + SSIM_C1, D = s1 + s2 + SSIM_C2;
            const float inv = 1.f / (Cv * D), rD = 1.f / D;
            const float qa = A / Cv, m = qa * (Bv / D);
            ss += m;
            l1 += fabsf(sx[ty + RAD][tx + RAD] - sy[ty + RAD][tx + RAD]);
            if (maps) {
                const size_t o = poff + (size_t)py * W + px;
                maps[o] = (2.f * mu2 * (Bv - A) - m * 2.f * mu1 * (D - Cv)) * inv;   // d m / d mu1  (E[x^2], E[xy] held fixed)
                maps[o + map_stride] = -(m * rD);                                    // d m / d E[x^2]
                maps[o + 2 * map_stride] = (2.f * qa) * rD;                          // d m / d E[xy]
            }
        }
    }
    l1 = wave_sum_hi(l1);
    ss = wave_sum_hi(ss);
    block_sum_post(red[0], l1, tid);
    block_sum_post(red[1], ss, tid);
    __syncthreads();
    if (tid == 0) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[blk] = make_float2(block_sum(red[0]), block_sum(red[1]));
    }
}

// one workgroup per image: fixed-order sum of that image's partials
__global__ __launch_bounds__(256) void k_reduce_partials(const float2* __restrict__ partial, int per_image, float scale, float2* __restrict__ sums)
{
    __shared__ float red[2][4];
    const int tid = threadIdx.x;
    const float2* p = partial + (size_t)blockIdx.x * per_image;
    float a = 0.f, b = 0.f;
    for (int i = tid; i < per_image; i += 256) {
        const float2 v = p[i];
        a += v.x;
        b += v.y;
    }
    a = wave_sum_hi(a);
    b = wave_sum_hi(b);
    block_sum_post(red[0], a, tid);
    block_sum_post(red[1], b, tid);
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = make_float2(scale * block_sum(red[0]), scale * block_sum(red[1]));
}

__global__ __launch_bounds__(256) void k_l1_ssim_bwd(int C, int H, int W, const float* __restrict__ img1, const float* __restrict__ img2,
                                                      const float* __restrict__ maps, size_t map_stride, Window win,
                                                      const float* __restrict__ g_l1, const float* __restrict__ g_ssim, int g_stride, float scale,
                                                      float* __restrict__ d_img1)
{
    __shared__ __attribute__((aligned(16))) float sm[3][HY][HXS];
    __shared__ __attribute__((aligned(16))) float hq[3][HY][TX];
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const size_t poff = (size_t)plane * H * W;
#pragma unroll
    for (int q = 0; q < 3; ++q) load_halo(sm[q], maps + q * map_stride + poff, H, W, x0, y0, tid);
    __syncthreads();
    horizontal_planes<3>(sm, hq, win, tid);   // the three derivative planes
    __syncthreads();
    const int tx = tid & 31, ty0 = (tid >> 5) * 2;
    float col[3][WIN + 1];
    load_columns(hq, tx, ty0, col);
    const int img = plane / C;   // dL/d(mean |x - y|) and dL/d(mean ssim) of this image; a missing one is zero
    float2 gi = make_float2(g_l1 ? g_l1[(size_t)img * g_stride] : 0.f, g_ssim ? g_ssim[(size_t)img * g_stride] : 0.f);
    gi.x *= scale;
    gi.y *= scale;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float cw[3];
        window_sums(col, win, j, cw);
        const float ca = cw[0], cb = cw[1], cc = cw[2];
        const int px = x0 + tx, py = y0 + ty0 + j;
        if (px < W && py < H) {
#pragma clang fp contract(off)   // (2 x cb and y cc rounded alike: they cancel exactly where cc == -2 cb, see k_l1_ssim_fwd)
            const size_t o = poff + (size_t)py * W + px;
            const float x = img1[o], y = img2[o];
            const float df = x - y;
            const float sgn = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
            d_img1[o] = gi.y * (ca + 2.f * x * cb + y * cc) + gi.x * sgn;
        }
    }
}

// ---- plain L1 -------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sgn_scaled(float d, float g) { return d > 0.f ? g : (d < 0.f ? -g : 0.f); }
// GRAD: also d_a <- gs * sign(a - b), the gradient for an upstream gradient of exactly 1 (gs = the forward's mean scale): a backward seeded
// with the constant 1 (loss.backward() on the loss itself) then has nothing left to launch
// FUSED (round 6): the reduction over the workgroups without a second launch and without a fence.  Every workgroup adds its partial, as 2^-30
// fixed point in bits 8 .. 62, and a 1 in the low byte to ONE 64-bit word with ONE returning atomic: the atomic is the only thing the workgroups
// share, so the one that reads back (grid - 1) arrivals holds every other partial in the value it got -- it writes the loss and leaves the word
// zero for the stream's next call.  Integer adds commute: the same bits whatever order the workgroups arrive in.  (Rounds 2 - 3 measured a
// ticket + fence + re-read of the partials at the price of the launch it replaced; here nothing is re-read.)  At most 255 workgroups.
// A partial takes that road only while it is below 2^17: 255 of them stay below 2^55, so the field never carries into bit 63 and the count, in
// the LOW byte, is never touched by a sum -- the last arriver is always found and always resets.  Anything else (!(tot < 2^17): a large
// partial, inf, NaN) goes to the stream's two side words first and sets bit 63 (an OR with release order, then the arrival add on the same
// address): word[1] takes partials below 2^26 as the same fixed point (255 of them fit 64 bits: the integer total, and with it the loss, is the
// bits one word would have given whenever the total fits 56 bits), word[2] takes the rest as a double (inf and NaN stay what they are).  The last
// arriver reads the side words only when it sees bit 63, so the usual image costs what it did.
constexpr float kL1Small = 131072.f, kL1Mid = 67108864.f;   // 2^17, 2^26
constexpr unsigned long long kL1Aside = 1ull << 63;
template <bool GRAD, bool FUSED>
__global__ __launch_bounds__(1024) void k_l1_fwd(long long n, const float* __restrict__ a, const float* __restrict__ b, float2* __restrict__ partial,
                                                  float gs, float* __restrict__ d_a, unsigned long long* __restrict__ word, float* __restrict__ sum)
{
    // (blockDim.x: 256 in the two-launch form; the one-launch form is held to 255 workgroups by its arrival count and takes WIDE ones -- with
    //  256 threads it ran one wave per SIMD, five dependent trips of two loads each: 7.6 us for 16 MB)
    __shared__ float red[16];
    const int tid = threadIdx.x, nt = (int)blockDim.x;
    const long long n4 = n >> 2;
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * nt + tid; i < n4; i += (long long)gridDim.x * nt) {
        const float4 u = ((const float4*)a)[i], v = ((const float4*)b)[i];
        const float dx = u.x - v.x, dy = u.y - v.y, dz = u.z - v.z, dw = u.w - v.w;
        s += (fabsf(dx) + fabsf(dy)) + (fabsf(dz) + fabsf(dw));
        if (GRAD) ((float4*)d_a)[i] = make_float4(sgn_scaled(dx, gs), sgn_scaled(dy, gs), sgn_scaled(dz, gs), sgn_scaled(dw, gs));
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) {
        const float d = a[(n4 << 2) + tid] - b[(n4 << 2) + tid];
        s += fabsf(d);
        if (GRAD) d_a[(n4 << 2) + tid] = sgn_scaled(d, gs);
    }
    s = wave_sum_hi(s);
    if ((tid & 63) == 63) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        float tot = (red[0] + red[1]) + (red[2] + red[3]);
        for (int w = 4; w < (nt >> 6); w += 4) tot += (red[w] + red[w + 1]) + (red[w + 2] + red[w + 3]);
        if constexpr (FUSED) {
            unsigned long long mine = 0;
            if (tot < kL1Small) {
                mine = (unsigned long long)((double)tot * 1073741824.0 + 0.5);
            } else {   // (NaN arrives here too)
                if (tot < kL1Mid) __hip_atomic_fetch_add(word + 1, (unsigned long long)((double)tot * 1073741824.0 + 0.5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else __hip_atomic_fetch_add((double*)(word + 2), (double)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_or(word, kL1Aside, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
            const unsigned long long old = __hip_atomic_fetch_add(word, (mine << 8) + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((old & 0xFFull) == (unsigned long long)(gridDim.x - 1)) {
                unsigned long long all = ((old & ~kL1Aside) >> 8) + mine;
                double rest = 0.0;
                if (old & kL1Aside) {
                    all += __hip_atomic_load(word + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                    rest = __hip_atomic_load((double*)(word + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(word + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store((double*)(word + 2), 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                const double fixed = (double)all * (1.0 / 1073741824.0);
                *sum = gs * (float)(fixed + rest);   // (rest == 0: the bits of `fixed`)
                __hip_atomic_store(word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the next call on this stream starts from zero)
            }
        } else {
            partial[blockIdx.x] = make_float2(tot, 0.f);
        }
    }
}
// (plain names for the launch sites: the event profile keys its table by the text of the launch expression)
constexpr auto k_l1_fwd_1 = &k_l1_fwd<false, true>;     // one launch, loss only
constexpr auto k_l1_fwd_1g = &k_l1_fwd<true, true>;     // one launch, loss + the unit-seed gradient image
constexpr auto k_l1_fwd_2 = &k_l1_fwd<false, false>;    // partials for k_l1_reduce
constexpr auto k_l1_fwd_2g = &k_l1_fwd<true, false>;
__global__ __launch_bounds__(256) void k_l1_reduce(const float2* __restrict__ partial, int count, float scale, float* __restrict__ sum)
{
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < count; i += 256) s += partial[i].x;
    s = wave_sum_hi(s);
    block_sum_post(red, s, tid);
    __syncthreads();
    if (tid == 0) *sum = scale * block_sum(red);
}
__global__ __launch_bounds__(256) void k_l1_bwd(long long n, const float* __restrict__ a, const float* __restrict__ b,
                                                 const float* __restrict__ g, float scale, float* __restrict__ d_a)
{
    const float gv = *g * scale;
    const long long n4 = n >> 2;
    const int tid = threadIdx.x;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
        const float4 u = ((const float4*)a)[i], v = ((const float4*)b)[i];
        ((float4*)d_a)[i] = make_float4(sgn_scaled(u.x - v.x, gv), sgn_scaled(u.y - v.y, gv), sgn_scaled(u.z - v.z, gv), sgn_scaled(u.w - v.w, gv));
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) {
        const long long i = (n4 << 2) + tid;
        d_a[i] = sgn_scaled(a[i] - b[i], gv);
    }
}

// ---- densification statistics -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_densify_stats(int P, const int* __restrict__ radii, const float* __restrict__ vgrad,
                                                        float* __restrict__ max_radii2D, float* __restrict__ accum, float* __restrict__ denom)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    if (r <= 0) return;
    max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
    const float gx = vgrad[3 * i], gy = vgrad[3 * i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.f;
}

// GaussianModel.add_densification_stats alone (scene/gaussian_model.py:517-519) with the caller's own bool filter: the form the reference's
// train.py:198 calls, rebound by patch_reference() (train.py:197's max_radii2D line is train.py's own torch code and stays there)
__global__ __launch_bounds__(256) void k_add_densify_stats(int P, const unsigned char* __restrict__ filter, const float* __restrict__ vgrad, int vstride,
                                                            float* __restrict__ accum, float* __restrict__ denom)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || !filter[i]) return;
    const float gx = vgrad[(size_t)vstride * i], gy = vgrad[(size_t)vstride * i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.f;
}

}  // namespace gls

// ---------------------------------------------------------------------------------------------------------------
using ssim_window::image_args_ok;
using ssim_window::make_window;
using ssim_window::tile_grid;
static const int kL1Blocks = 1024;

extern "C" {

int gls_abi_version(void) { return GLS_ABI_VERSION; }
const char* gls_last_error(void) { return g_err; }

int64_t gls_partial_floats(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 2 * kL1Blocks;
    const int64_t tiles = ssim_window::tile_count(B, C, H, W);
    return 2 * (tiles > kL1Blocks ? tiles : kL1Blocks);
}

int gls_l1_ssim_forward(int32_t B, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, float scale, float* sums,
                        float* maps, float* partial, void* stream_)
{
    if (!image_args_ok(B, C, H, W)) return fail(GLS_E_ARG, "bad image shape (%d,%d,%d,%d)", B, C, H, W);
    if (!img1 || !img2 || !sums || !partial) return fail(GLS_E_ARG, "null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid = tile_grid(B, C, H, W);
    const size_t stride = (size_t)B * C * H * W;
    PROF_LAUNCH(gls::k_l1_ssim_fwd, grid, dim3(256), 0, stream, H, W, img1, img2, make_window(), maps, stride, (float2*)partial);
    LAUNCH_CHECK(GLS_E_HIP, "k_l1_ssim_fwd");
    PROF_LAUNCH(gls::k_reduce_partials, dim3(B), dim3(256), 0, stream, (const float2*)partial, (int)(grid.x * grid.y * C), scale, (float2*)sums);
    LAUNCH_CHECK(GLS_E_HIP, "k_reduce_partials");
    return GLS_OK;
}

static int l1_ssim_backward_impl(int32_t B, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* maps,
                                 const float* g_l1, const float* g_ssim, int g_stride, float scale, float* d_img1, void* stream_)
{
    if (!image_args_ok(B, C, H, W)) return fail(GLS_E_ARG, "bad image shape (%d,%d,%d,%d)", B, C, H, W);
    if (!img1 || !img2 || !maps || !d_img1 || g_stride < 0) return fail(GLS_E_ARG, "null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid = tile_grid(B, C, H, W);
    const size_t stride = (size_t)B * C * H * W;
    PROF_LAUNCH(gls::k_l1_ssim_bwd, grid, dim3(256), 0, stream, C, H, W, img1, img2, maps, stride, make_window(), g_l1, g_ssim, g_stride, scale, d_img1);
    LAUNCH_CHECK(GLS_E_HIP, "k_l1_ssim_bwd");
    return GLS_OK;
}

int gls_l1_ssim_backward(int32_t B, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* maps,
                         const float* g, float scale, float* d_img1, void* stream_)
{
    if (!g) return fail(GLS_E_ARG, "null pointer");
    return l1_ssim_backward_impl(B, C, H, W, img1, img2, maps, g, g + 1, 2, scale, d_img1, stream_);
}

int gls_l1_ssim_backward_split(int32_t B, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* maps,
                               const float* g_l1, const float* g_ssim, int32_t g_stride, float scale, float* d_img1, void* stream_)
{
    return l1_ssim_backward_impl(B, C, H, W, img1, img2, maps, g_l1, g_ssim, g_stride, scale, d_img1, stream_);
}

// the accumulator word of the fused L1 forward and its two side words, one group of kL1Group per stream (calls on a stream are ordered,
// concurrent streams never share a group)
static unsigned long long* l1_word_for(hipStream_t stream)
{
    constexpr int kWords = 64, kL1Group = 4;
    static std::mutex mu;
    static std::vector<hipStream_t> owners;
    static std::vector<int> owner_dev;                  // (the table is keyed by (device, stream))
    static std::vector<unsigned long long*> bases;      // one block of words per device
    static std::vector<int> base_dev;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    unsigned long long* b = nullptr;
    for (size_t i = 0; i < bases.size(); ++i)
        if (base_dev[i] == dev) b = bases[i];
    if (!b) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;   // (no allocation inside a capture: the two-launch form)
        if (hipMalloc((void**)&b, kWords * kL1Group * sizeof(unsigned long long)) != hipSuccess) return nullptr;
        if (hipMemset(b, 0, kWords * kL1Group * sizeof(unsigned long long)) != hipSuccess) return nullptr;
        bases.push_back(b); base_dev.push_back(dev);
    }
    int slot = -1, used = 0;
    for (size_t i = 0; i < owners.size(); ++i) {
        if (owner_dev[i] != dev) continue;
        if (owners[i] == stream) slot = used;
        ++used;
    }
    if (slot < 0) {
        if (used >= kWords) return nullptr;   // more streams than words: the two-launch form
        owners.push_back(stream); owner_dev.push_back(dev);
        slot = used;
    }
    return b + slot * kL1Group;
}

static int l1_forward_impl(int64_t n, const float* a, const float* b, float scale, float* sum, float* partial, float* d_a, bool grad, void* stream_)
{
    if (n < 0 || !sum || !partial || (n > 0 && (!a || !b || (grad && !d_a)))) return fail(GLS_E_ARG, "bad arguments");
    if ((((uintptr_t)a) | ((uintptr_t)b) | (grad ? (uintptr_t)d_a : 0)) & 15) return fail(GLS_E_ARG, "buffers must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    int blocks = (int)(((n >> 2) + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > kL1Blocks ? kL1Blocks : blocks);
    // one launch (round 6): <= 255 workgroups, each adds its partial to the stream's accumulator word with one returning atomic; the last arriver writes the loss
    static const bool fused_on = [] { const char* e = getenv("GLS_L1_FUSED"); return !(e && e[0] == '0'); }();
    unsigned long long* word = (fused_on && n < (1ll << 26)) ? l1_word_for(stream) : nullptr;
    if (word) {
        constexpr int fmax = 255, fthreads = 1024;   // workgroups (at most) and threads of each
        const int wide = (int)(((n >> 2) + fthreads - 1) / fthreads);
        const int fb = wide < 1 ? 1 : (wide > fmax ? fmax : wide);
        if (grad) PROF_LAUNCH(gls::k_l1_fwd_1g, dim3(fb), dim3(fthreads), 0, stream, (long long)n, a, b, (float2*)partial, scale, d_a, word, sum);
        else PROF_LAUNCH(gls::k_l1_fwd_1, dim3(fb), dim3(fthreads), 0, stream, (long long)n, a, b, (float2*)partial, scale, (float*)nullptr, word, sum);
        LAUNCH_CHECK(GLS_E_HIP, "k_l1_fwd");
        return GLS_OK;
    }
    if (grad) PROF_LAUNCH(gls::k_l1_fwd_2g, dim3(blocks), dim3(256), 0, stream, (long long)n, a, b, (float2*)partial, scale, d_a, (unsigned long long*)nullptr, (float*)nullptr);
    else PROF_LAUNCH(gls::k_l1_fwd_2, dim3(blocks), dim3(256), 0, stream, (long long)n, a, b, (float2*)partial, scale, (float*)nullptr, (unsigned long long*)nullptr, (float*)nullptr);
    LAUNCH_CHECK(GLS_E_HIP, "k_l1_fwd");
    PROF_LAUNCH(gls::k_l1_reduce, dim3(1), dim3(256), 0, stream, (const float2*)partial, blocks, scale, sum);
    LAUNCH_CHECK(GLS_E_HIP, "k_l1_reduce");
    return GLS_OK;
}

int gls_l1_forward(int64_t n, const float* a, const float* b, float scale, float* sum, float* partial, void* stream_)
{
    return l1_forward_impl(n, a, b, scale, sum, partial, nullptr, false, stream_);
}

int gls_l1_forward_grad(int64_t n, const float* a, const float* b, float scale, float* sum, float* partial, float* d_a, void* stream_)
{
    return l1_forward_impl(n, a, b, scale, sum, partial, d_a, true, stream_);
}

int gls_l1_backward(int64_t n, const float* a, const float* b, const float* g, float scale, float* d_a, void* stream_)
{
    if (n < 0 || !g || (n > 0 && (!a || !b || !d_a))) return fail(GLS_E_ARG, "bad arguments");
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)d_a)) & 15) return fail(GLS_E_ARG, "buffers must be 16-byte aligned");
    if (n == 0) return GLS_OK;
    hipStream_t stream = (hipStream_t)stream_;
    int blocks = (int)(((n >> 2) + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    PROF_LAUNCH(gls::k_l1_bwd, dim3(blocks), dim3(256), 0, stream, (long long)n, a, b, g, scale, d_a);
    LAUNCH_CHECK(GLS_E_HIP, "k_l1_bwd");
    return GLS_OK;
}

int gls_densification_stats(int32_t P, const int32_t* radii, const float* viewspace_grad, float* max_radii2D, float* xyz_gradient_accum,
                            float* denom, void* stream_)
{
    if (P < 0) return fail(GLS_E_ARG, "P < 0");
    if (P == 0) return GLS_OK;
    if (!radii || !viewspace_grad || !max_radii2D || !xyz_gradient_accum || !denom) return fail(GLS_E_ARG, "null pointer");
    PROF_LAUNCH(gls::k_densify_stats, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, P, radii, viewspace_grad,
                       max_radii2D, xyz_gradient_accum, denom);
    LAUNCH_CHECK(GLS_E_HIP, "k_densify_stats");
    return GLS_OK;
}

int gls_add_densification_stats(int32_t P, const uint8_t* update_filter, const float* viewspace_grad, int32_t grad_stride, float* xyz_gradient_accum,
                                float* denom, void* stream_)
{
    if (P < 0 || grad_stride < 2) return fail(GLS_E_ARG, "P < 0 or grad_stride < 2");
    if (P == 0) return GLS_OK;
    if (!update_filter || !viewspace_grad || !xyz_gradient_accum || !denom) return fail(GLS_E_ARG, "null pointer");
    PROF_LAUNCH(gls::k_add_densify_stats, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, P, update_filter, viewspace_grad, grad_stride,
                       xyz_gradient_accum, denom);
    LAUNCH_CHECK(GLS_E_HIP, "k_add_densify_stats");
    return GLS_OK;
}

LPROF_EXPORTS(gls)

}  // extern "C"

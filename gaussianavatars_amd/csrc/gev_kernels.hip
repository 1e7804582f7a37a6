// gev_kernels.hip -- evaluation and export (include/gev.h): the statistics of an image pair that training_report (train.py:256-309) and
// metrics.py take with 30 - 40 composed torch launches, in two; and the bytes render.py:41 writes, in one.
//
// k_pair_stats forms the five windowed moments of a tile with the window of ssim_window.h, the one gls::k_l1_ssim_fwd (gls_kernels.hip) is
// built from, and the tile's sums go out as one fixed-order partial.  Its own: the halo load reads either layout of include/gev.h and applies
// the load transform ONCE per pixel, there are no derivative planes, the SSIM map is A * Bv * (1 / (Cv * D)) (gls forms a product of two
// quotients: DESIGN.md section 17), and the tile also sums (a-b)^2 -- in fp64, because PSNR is new here and has no tolerance to inherit.
// k_reduce_accumulate adds the tiles of every plane in fp64 and, as its last act, forms the image's figures and adds them to the
// device-resident running sums.
// Built with -ffp-contract=off: to_byte's multiply and add must round separately (the bytes are torch's bytes).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gev.h"
#include "launch_prof.h"
#include "lib_common.h"
#include "ssim_window.h"
#include "wave_reduce.h"

namespace gev {

using namespace ssim_window;
using wave_reduce::wave_sum_hi;   // sum over the 64 lanes, valid in lane 63 (float and double)
static_assert(WIN == GEV_SSIM_WINDOW, "include/gev.h publishes the window ssim_window.h applies");

// one tile's sums: |a-b| and the SSIM map in fp32 (the arithmetic of gls_l1_ssim_forward), (a-b)^2 in fp64
struct TileSums {
    float l1, ss;
    double sq;
};

// render.py:41 for one value: mul(255), add_(0.5), clamp_(0, 255), to(uint8).  Four roundings, none fused (-ffp-contract=off).  fmaxf sends a
// NaN to 0 and the clamp leaves nothing outside [0, 255] for the conversion, so no input faults or is undefined here.
__device__ __forceinline__ unsigned to_byte(float x)
{
    float v = x * 255.f;
    v = v + 0.5f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (unsigned)(int)v;
}

__device__ __forceinline__ float transformed(float x, int transform)
{
    if (transform == GEV_CLAMP) return fminf(fmaxf(x, 0.f), 1.f);
    if (transform == GEV_PNG8) return (float)to_byte(x) / 255.f;
    return x;
}

// the halo of one plane of either layout, transformed ONCE per pixel
__device__ __forceinline__ void load_halo(float (*dst)[HXS], const void* __restrict__ img, int layout, int transform, int C, int H, int W, int plane,
                                          int x0, int y0, int tid)
{
    const int b = plane / C, c = plane - b * C;
    const float* __restrict__ fplane = (const float*)img + (size_t)plane * H * W;
    const unsigned char* __restrict__ bimg = (const unsigned char*)img + (size_t)b * H * W * C + c;
    ssim_window::load_halo(dst, H, W, x0, y0, tid, [=](int gy, int gx) {
        const size_t px = (size_t)gy * W + gx;
        return layout == GEV_U8_INTERLEAVED ? (float)bimg[px * C] / 255.f : transformed(fplane[px], transform);
    });
}

__global__ __launch_bounds__(256) void k_pair_stats(int C, int H, int W, const void* __restrict__ img1, int layout1, const void* __restrict__ img2,
                                                     int layout2, int transform, Window win, TileSums* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float sx[HY][HXS], sy[HY][HXS];
    __shared__ __attribute__((aligned(16))) float hq[5][HY][TX];
    __shared__ float red[2][4];
    __shared__ double redd[4];
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    load_halo(sx, img1, layout1, transform, C, H, W, plane, x0, y0, tid);
    load_halo(sy, img2, layout2, transform, C, H, W, plane, x0, y0, tid);
    __syncthreads();
    horizontal_pair(sx, sy, hq, win, tid);
    __syncthreads();
    const int tx = tid & 31, ty0 = (tid >> 5) * 2;   // vertical taps: column tx, rows ty0 and ty0 + 1
    float col[5][WIN + 1];
    load_columns(hq, tx, ty0, col);
    float l1 = 0.f, ss = 0.f;
    double sq = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float e[5];   // E[x], E[y], E[x^2], E[y^2], E[xy]
        window_sums(col, win, j, e);
        const float mu1 = e[0], mu2 = e[1], e11 = e[2], e22 = e[3], e12 = e[4];
        const int ty = ty0 + j, px = x0 + tx, py = y0 + ty;
        if (px < W && py < H) {
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
            const float A = 2.f * mu12 + SSIM_C1, Bv = 2.f * s12 + SSIM_C2;
            const float Cv = mu1_sq + mu2_sq + SSIM_C1, D = s1 + s2 + SSIM_C2;
            ss += A * Bv * (1.f / (Cv * D));
            const float x = sx[ty + RAD][tx + RAD], y = sy[ty + RAD][tx + RAD];
            l1 += fabsf(x - y);
            const double d = (double)x - (double)y;
            sq += d * d;
        }
    }
    l1 = wave_sum_hi(l1);
    ss = wave_sum_hi(ss);
    sq = wave_sum_hi(sq);
    block_sum_post(red[0], l1, tid);
    block_sum_post(red[1], ss, tid);
    block_sum_post(redd, sq, tid);
    __syncthreads();
    if (tid == 0) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        TileSums t;
        t.l1 = block_sum(red[0]);
        t.ss = block_sum(red[1]);
        t.sq = block_sum(redd);
        partial[blk] = t;
    }
}

// ONE workgroup: wave w adds the tiles of planes w, w + 4, ... (a lane its every 64th tile, then the lanes by DPP: a fixed order), writes the
// plane's three sums, and thread 0 then forms every image's figures from them and adds them to the running sums (include/gev.h: gev_accumulate)
__global__ __launch_bounds__(256) void k_reduce_accumulate(const TileSums* __restrict__ partial, int B, int C, int tiles, double hw, int psnr_mode,
                                                            double* plane_sums, float* __restrict__ per_view, int row, double* __restrict__ acc)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int planes = B * C;
    for (int p = wave; p < planes; p += 4) {
        const TileSums* __restrict__ t = partial + (size_t)p * tiles;
        double l1 = 0.0, sq = 0.0, ss = 0.0;
        for (int i = lane; i < tiles; i += 64) {
            const TileSums v = t[i];
            l1 += (double)v.l1;
            sq += v.sq;
            ss += (double)v.ss;
        }
        l1 = wave_sum_hi(l1);
        sq = wave_sum_hi(sq);
        ss = wave_sum_hi(ss);
        if (lane == 63) {
            plane_sums[3 * (size_t)p] = l1;
            plane_sums[3 * (size_t)p + 1] = sq;
            plane_sums[3 * (size_t)p + 2] = ss;
        }
    }
    if (!per_view && !acc) return;
    __threadfence_block();
    __syncthreads();
    if (tid != 0) return;
    for (int i = 0; i < B; ++i) {
        double l1 = 0.0, sq = 0.0, ss = 0.0, ps = 0.0;
        for (int c = 0; c < C; ++c) {
            const double* s = plane_sums + 3 * ((size_t)i * C + c);
            l1 += s[0];
            sq += s[1];
            ss += s[2];
            ps += -10.0 * log10(s[1] / hw);   // = 20 log10(1 / sqrt(mse)); mse = 0 gives +inf, as the reference
        }
        const double n = hw * (double)C;
        const float f_l1 = (float)(l1 / n), f_ss = (float)(ss / n);
        const float f_ps = (float)(psnr_mode == GEV_PSNR_PER_IMAGE ? -10.0 * log10(sq / n) : ps / (double)C);
        if (per_view) {
            float* o = per_view + 3 * ((size_t)row + i);
            o[0] = f_l1;
            o[1] = f_ps;
            o[2] = f_ss;
        }
        if (acc) {
            acc[0] += (double)f_l1;
            acc[1] += (double)f_ps;
            acc[2] += (double)f_ss;
            acc[3] += 1.0;
        }
    }
}

// ---- the 8-bit frame ------------------------------------------------------------------------------------------------
// C == 3, H*W a multiple of 4: a thread takes four neighbouring pixels -- one 16-byte load from each of the three planes, twelve bytes out
// as three packed words.  blockIdx.y selects the image (0: src0 -> dst0, 1: src1 -> dst1).
__global__ __launch_bounds__(256) void k_to_u8_rgb4(long long groups, int HW, const float* __restrict__ src0, unsigned char* __restrict__ dst0,
                                                     const float* __restrict__ src1, unsigned char* __restrict__ dst1)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const float* __restrict__ src = blockIdx.y ? src1 : src0;
    unsigned char* __restrict__ dst = blockIdx.y ? dst1 : dst0;
    const long long p = g * 4, b = p / HW, q = p - b * HW;
    const float* base = src + (size_t)b * 3 * HW + q;
    const float4 r = *reinterpret_cast<const float4*>(base);
    const float4 gr = *reinterpret_cast<const float4*>(base + HW);
    const float4 bl = *reinterpret_cast<const float4*>(base + 2 * (size_t)HW);
    const unsigned w0 = to_byte(r.x) | (to_byte(gr.x) << 8) | (to_byte(bl.x) << 16) | (to_byte(r.y) << 24);
    const unsigned w1 = to_byte(gr.y) | (to_byte(bl.y) << 8) | (to_byte(r.z) << 16) | (to_byte(gr.z) << 24);
    const unsigned w2 = to_byte(bl.z) | (to_byte(r.w) << 8) | (to_byte(gr.w) << 16) | (to_byte(bl.w) << 24);
    unsigned* o = reinterpret_cast<unsigned*>(dst + (size_t)p * 3);
    o[0] = w0;
    o[1] = w1;
    o[2] = w2;
}
// any other shape: a thread takes one pixel, its C channels
__global__ __launch_bounds__(256) void k_to_u8_any(long long pixels, int C, int HW, const float* __restrict__ src0, unsigned char* __restrict__ dst0,
                                                    const float* __restrict__ src1, unsigned char* __restrict__ dst1)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const float* __restrict__ src = blockIdx.y ? src1 : src0;
    unsigned char* __restrict__ dst = blockIdx.y ? dst1 : dst0;
    const long long b = p / HW, q = p - b * HW;
    const float* base = src + (size_t)b * C * HW + q;
    unsigned char* o = dst + (size_t)p * C;
    for (int c = 0; c < C; ++c) o[c] = (unsigned char)to_byte(base[(size_t)c * HW]);
}

}  // namespace gev

// ---------------------------------------------------------------------------------------------------------------
using ssim_window::image_args_ok;
using ssim_window::make_window;
static bool layout_ok(int32_t l) { return l == GEV_F32_PLANAR || l == GEV_U8_INTERLEAVED; }

static int stats_impl(int32_t B, int32_t C, int32_t H, int32_t W, const void* a, int32_t a_layout, const void* b, int32_t b_layout, int32_t transform,
                      int32_t psnr_mode, double* plane_sums, float* partial, float* per_view, int32_t row, double* acc, void* stream_)
{
    if (!image_args_ok(B, C, H, W)) return fail(GEV_E_ARG, "bad image shape (%d,%d,%d,%d)", B, C, H, W);
    if (!a || !b || !plane_sums || !partial) return fail(GEV_E_ARG, "null pointer");
    if (!layout_ok(a_layout) || !layout_ok(b_layout)) return fail(GEV_E_ARG, "unknown layout (%d, %d)", a_layout, b_layout);
    if (transform != GEV_RAW && transform != GEV_CLAMP && transform != GEV_PNG8) return fail(GEV_E_ARG, "unknown transform %d", transform);
    if (psnr_mode != GEV_PSNR_PER_CHANNEL && psnr_mode != GEV_PSNR_PER_IMAGE) return fail(GEV_E_ARG, "unknown psnr mode %d", psnr_mode);
    if (row < 0) return fail(GEV_E_ARG, "row < 0");
    if ((((uintptr_t)partial) | ((uintptr_t)plane_sums) | ((uintptr_t)acc)) & 7) return fail(GEV_E_ARG, "partial, plane_sums and acc must be 8-byte aligned");
    if ((a_layout == GEV_F32_PLANAR && ((uintptr_t)a & 3)) || (b_layout == GEV_F32_PLANAR && ((uintptr_t)b & 3)) || ((uintptr_t)per_view & 3))
        return fail(GEV_E_ARG, "float buffers must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid = ssim_window::tile_grid(B, C, H, W);
    PROF_LAUNCH(gev::k_pair_stats, grid, dim3(256), 0, stream, C, H, W, a, a_layout, b, b_layout, transform, make_window(), (gev::TileSums*)partial);
    LAUNCH_CHECK(GEV_E_HIP, "k_pair_stats");
    PROF_LAUNCH(gev::k_reduce_accumulate, dim3(1), dim3(256), 0, stream, (const gev::TileSums*)partial, B, C, (int)(grid.x * grid.y),
                (double)H * (double)W, psnr_mode, plane_sums, per_view, row, acc);
    LAUNCH_CHECK(GEV_E_HIP, "k_reduce_accumulate");
    return GEV_OK;
}

extern "C" {

int gev_abi_version(void) { return GEV_ABI_VERSION; }
const char* gev_last_error(void) { return g_err; }

int64_t gev_partial_floats(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return ssim_window::tile_count(B, C, H, W) * (int64_t)(sizeof(gev::TileSums) / sizeof(float));
}

int gev_pair_stats(int32_t B, int32_t C, int32_t H, int32_t W, const void* a, int32_t a_layout, const void* b, int32_t b_layout, int32_t transform,
                   double* plane_sums, float* partial, void* stream)
{
    return stats_impl(B, C, H, W, a, a_layout, b, b_layout, transform, GEV_PSNR_PER_CHANNEL, plane_sums, partial, nullptr, 0, nullptr, stream);
}

int gev_accumulate(int32_t B, int32_t C, int32_t H, int32_t W, const void* a, int32_t a_layout, const void* b, int32_t b_layout, int32_t transform,
                   int32_t psnr_mode, double* plane_sums, float* partial, float* per_view, int32_t row, double* acc, void* stream)
{
    return stats_impl(B, C, H, W, a, a_layout, b, b_layout, transform, psnr_mode, plane_sums, partial, per_view, row, acc, stream);
}

int gev_to_u8(int32_t B, int32_t C, int32_t H, int32_t W, const float* src, uint8_t* dst, const float* src2, uint8_t* dst2, void* stream_)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(GEV_E_ARG, "bad image shape (%d,%d,%d,%d)", B, C, H, W);
    if (!src || !dst || (!src2) != (!dst2)) return fail(GEV_E_ARG, "null pointer");
    if (((uintptr_t)src | (uintptr_t)src2) & 3) return fail(GEV_E_ARG, "float buffers must be 4-byte aligned");
    const int64_t HW = (int64_t)H * W, pixels = HW * B;
    if (HW > INT32_MAX || pixels > (int64_t)INT32_MAX * 256) return fail(GEV_E_ARG, "image too large");
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned sets = src2 ? 2u : 1u;
    const bool vec = C == 3 && (HW & 3) == 0 && !(((uintptr_t)src | (uintptr_t)src2) & 15) && !(((uintptr_t)dst | (uintptr_t)dst2) & 3);
    if (vec) {
        const long long groups = pixels / 4;
        PROF_LAUNCH(gev::k_to_u8_rgb4, dim3((unsigned)((groups + 255) / 256), sets), dim3(256), 0, stream, groups, (int)HW, src, dst, src2, dst2);
        LAUNCH_CHECK(GEV_E_HIP, "k_to_u8_rgb4");
    } else {
        PROF_LAUNCH(gev::k_to_u8_any, dim3((unsigned)((pixels + 255) / 256), sets), dim3(256), 0, stream, (long long)pixels, (int)C, (int)HW, src, dst, src2,
                    dst2);
        LAUNCH_CHECK(GEV_E_HIP, "k_to_u8_any");
    }
    return GEV_OK;
}

LPROF_EXPORTS(gev)

}  // extern "C"

// gev_kernels.hip -- evaluation and export (include/gev.h): the statistics of an image pair that training_report (train.py:256-309) and
// metrics.py take with 30 - 40 composed torch launches, in two; and the bytes render.py:41 writes, in one.
//
// k_pair_stats has the structure of gls::k_l1_ssim_fwd (gls_kernels.hip): per 32x16 output tile the 42x26 halo of both images goes to LDS
// once (zero padding as F.conv2d(padding=5)), the five windowed moments are formed separably (11 horizontal taps into LDS, 11 vertical taps
// in registers, every output adding its taps in the order k = 0 .. 10), and the tile's sums go out as one fixed-order partial.  What differs:
// the halo load reads either layout of include/gev.h and applies the load transform ONCE per pixel, there are no derivative planes, and the
// tile also sums (a-b)^2 -- in fp64, because PSNR is new here and has no tolerance to inherit.  k_reduce_accumulate adds the tiles of every
// plane in fp64 and, as its last act, forms the image's figures and adds them to the device-resident running sums.
// Built with -ffp-contract=off: to_byte's multiply and add must round separately (the bytes are torch's bytes).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gev.h"
#include "launch_prof.h"
#include "lib_common.h"

namespace gev {

constexpr int WIN = GEV_SSIM_WINDOW, RAD = WIN / 2;
constexpr int TX = 32, TY = 16, HX = TX + 2 * RAD, HY = TY + 2 * RAD, HXS = HX + 2;   // (row stride 44: 16-byte rows)
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

struct Window {
    float w[WIN];
};
// one tile's sums: |a-b| and the SSIM map in fp32 (the arithmetic of gls_l1_ssim_forward), (a-b)^2 in fp64
struct TileSums {
    float l1, ss;
    double sq;
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_d(double v)   // (the two halves move separately; a lane outside the row mask reads +0.0, as in dpp_f)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
// sum over the 64 lanes, valid in lane 63
__device__ __forceinline__ float wave_sum_hi(float v)
{
    v += dpp_f<0xB1, 0xf>(v);
    v += dpp_f<0x4E, 0xf>(v);
    v += dpp_f<0x141, 0xf>(v);
    v += dpp_f<0x140, 0xf>(v);
    v += dpp_f<0x142, 0xa>(v);
    v += dpp_f<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ double wave_sum_hi(double v)
{
    v += dpp_d<0xB1, 0xf>(v);
    v += dpp_d<0x4E, 0xf>(v);
    v += dpp_d<0x141, 0xf>(v);
    v += dpp_d<0x140, 0xf>(v);
    v += dpp_d<0x142, 0xa>(v);
    v += dpp_d<0x143, 0xc>(v);
    return v;
}

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

// loads the (HY x HX) halo of one plane into LDS, transformed, zero outside the image
__device__ __forceinline__ void load_halo(float (*dst)[HXS], const void* __restrict__ img, int layout, int transform, int C, int H, int W, int plane,
                                          int x0, int y0, int tid)
{
    const int b = plane / C, c = plane - b * C;
    const float* __restrict__ fplane = (const float*)img + (size_t)plane * H * W;
    const unsigned char* __restrict__ bimg = (const unsigned char*)img + (size_t)b * H * W * C + c;
    for (int i = tid; i < HY * HX; i += 256) {
        const int r = i / HX, col = i - r * HX;
        const int gy = y0 + r - RAD, gx = x0 + col - RAD;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t px = (size_t)gy * W + gx;
            v = layout == GEV_U8_INTERLEAVED ? (float)bimg[px * C] / 255.f : transformed(fplane[px], transform);
        }
        dst[r][col] = v;
    }
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
    if (tid < HY * (TX / 4)) {   // horizontal taps: row r, columns c0 .. c0 + 3
        const int r = tid >> 3, c0 = (tid & 7) * 4;
        float xs[WIN + 3], ys[WIN + 3];
#pragma unroll
        for (int k = 0; k < WIN + 3; ++k) { xs[k] = sx[r][c0 + k]; ys[k] = sy[r][c0 + k]; }
        float o[5][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float x = xs[j + k], y = ys[j + k], w = win.w[k];
                a += w * x;
                b += w * y;
                aa += w * (x * x);
                bb += w * (y * y);
                ab += w * (x * y);
            }
            o[0][j] = a; o[1][j] = b; o[2][j] = aa; o[3][j] = bb; o[4][j] = ab;
        }
#pragma unroll
        for (int m = 0; m < 5; ++m) *reinterpret_cast<float4*>(&hq[m][r][c0]) = make_float4(o[m][0], o[m][1], o[m][2], o[m][3]);
    }
    __syncthreads();
    const int tx = tid & 31, ty0 = (tid >> 5) * 2;   // vertical taps: column tx, rows ty0 and ty0 + 1
    float col[5][WIN + 1];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int k = 0; k < WIN + 1; ++k) col[m][k] = hq[m][ty0 + k][tx];
    float l1 = 0.f, ss = 0.f;
    double sq = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float w = win.w[k];
            mu1 += w * col[0][j + k];
            mu2 += w * col[1][j + k];
            e11 += w * col[2][j + k];
            e22 += w * col[3][j + k];
            e12 += w * col[4][j + k];
        }
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
    if ((tid & 63) == 63) { red[0][tid >> 6] = l1; red[1][tid >> 6] = ss; redd[tid >> 6] = sq; }
    __syncthreads();
    if (tid == 0) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        TileSums t;
        t.l1 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        t.ss = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        t.sq = (redd[0] + redd[1]) + (redd[2] + redd[3]);
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
static gev::Window make_window()
{
    // utils/loss_utils.py:23-25: exp(-(x - 5)^2 / (2 * 1.5^2)) held in fp32, divided by its fp32 sum
    gev::Window w;
    float sum = 0.f;
    for (int x = 0; x < gev::WIN; ++x) {
        w.w[x] = (float)std::exp(-(double)((x - gev::RAD) * (x - gev::RAD)) / (2.0 * 1.5 * 1.5));
        sum += w.w[x];
    }
    for (int x = 0; x < gev::WIN; ++x) w.w[x] /= sum;
    return w;
}

static bool image_args_ok(int32_t B, int32_t C, int32_t H, int32_t W)
{
    return B > 0 && C > 0 && H > 0 && W > 0 && (int64_t)B * C <= 65535 && (H + gev::TY - 1) / gev::TY <= 65535;
}
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
    const dim3 grid((W + gev::TX - 1) / gev::TX, (H + gev::TY - 1) / gev::TY, B * C);
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
    const int64_t tiles = (int64_t)((W + gev::TX - 1) / gev::TX) * ((H + gev::TY - 1) / gev::TY) * B * C;
    return tiles * (int64_t)(sizeof(gev::TileSums) / sizeof(float));
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

// ssim_window.h -- the separable 11-tap Gaussian window of SSIM over a 32 x 16 output tile, once: gls::k_l1_ssim_fwd, gls::k_l1_ssim_bwd
// (gls_kernels.hip) and gev::k_pair_stats (gev_kernels.hip) are built from the pieces below, 256 threads per tile.
//
// The scheme.  Per 32 x 16 output tile the 42 x 26 halo of every input plane goes to LDS once (load_halo: zero outside the image, the
// padding of F.conv2d(padding=5); 2.1 x the tile's pixels, where a 16 x 16 tile's 26 x 26 halo was 2.6 x).  The window is applied separably
// with REGISTER-BLOCKED taps: a thread of the horizontal pass owns four neighbouring columns of a halo row and reads their 14 inputs once
// (28 LDS reads for four outputs where one output at a time took 22 each) and stores a float4 per plane into hq; a thread of the vertical
// pass owns two neighbouring rows of a column (load_columns: 12 reads per plane for two outputs instead of 22) and forms each row's sums
// in registers (window_sums).  Every output adds its eleven taps in the order k = 0 .. 10, so the values are the bits of a kernel that takes
// one output at a time.  What a kernel does with the windowed sums -- the SSIM map, its derivative planes, the squared error -- is its own
// and stays in its .hip file, as do its __launch_bounds__.
// Measured when the tile went from 16 x 16 to 32 x 16 (rocprofv3, train workload): k_l1_ssim_fwd 24.4 -> 24.2 us, k_l1_ssim_bwd
// 25.4 -> 22.6 us -- the LDS reads were not what bounds the pair: the forward writes 15.9 MB of derivative planes and the backward reads them
// back with their halos (~38 MB each way per kernel at ~3 TB/s).
//
// Contraction.  Everything on the device side is __forceinline__ code in this header, so each translation unit compiles it under its own
// -ffp-contract: libgls (fast-honor-pragmas) fuses w * x into the running sums, libgev (off) rounds the product and the sum separately.
// That is on purpose -- it is what each library did with its own copy, and their results are pinned bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace ssim_window {

// (WIN is the header's own: include/gls.h and include/gev.h each publish it as <LIB>_SSIM_WINDOW and each library asserts that they agree)
constexpr int WIN = 11, RAD = WIN / 2;
constexpr int TX = 32, TY = 16, HX = TX + 2 * RAD, HY = TY + 2 * RAD, HXS = HX + 2;   // (row stride 44: 16-byte rows)
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

struct Window {
    float w[WIN];
};

// ---- host ------------------------------------------------------------------------------------------------------------
static inline Window make_window()
{
    // utils/loss_utils.py:23-25: exp(-(x - 5)^2 / (2 * 1.5^2)) held in fp32, divided by its fp32 sum
    Window w;
    float sum = 0.f;
    for (int x = 0; x < WIN; ++x) {
        w.w[x] = (float)std::exp(-(double)((x - RAD) * (x - RAD)) / (2.0 * 1.5 * 1.5));
        sum += w.w[x];
    }
    for (int x = 0; x < WIN; ++x) w.w[x] /= sum;
    return w;
}

// one workgroup per tile per plane: (W / 32, H / 16, B C)
static inline int tiles_x(int32_t W) { return (W + TX - 1) / TX; }
static inline int tiles_y(int32_t H) { return (H + TY - 1) / TY; }
static inline dim3 tile_grid(int32_t B, int32_t C, int32_t H, int32_t W) { return dim3(tiles_x(W), tiles_y(H), B * C); }
static inline int64_t tile_count(int32_t B, int32_t C, int32_t H, int32_t W) { return (int64_t)tiles_x(W) * tiles_y(H) * B * C; }
// a shape tile_grid() can launch
static inline bool image_args_ok(int32_t B, int32_t C, int32_t H, int32_t W)
{
    return B > 0 && C > 0 && H > 0 && W > 0 && (int64_t)B * C <= 65535 && tiles_y(H) <= 65535;
}

// ---- device: 256 threads, thread tid -------------------------------------------------------------------------------------
// loads the (HY x HX) halo of the tile at (x0, y0) into LDS, zero outside the image; fetch(gy, gx) reads a pixel known to be inside it
template <class Fetch>
__device__ __forceinline__ void load_halo(float (*dst)[HXS], int H, int W, int x0, int y0, int tid, Fetch fetch)
{
    for (int i = tid; i < HY * HX; i += 256) {
        const int r = i / HX, c = i - r * HX;
        const int gy = y0 + r - RAD, gx = x0 + c - RAD;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        dst[r][c] = in ? fetch(gy, gx) : 0.f;
    }
}

// horizontal taps of an image pair: row r of the halo, columns c0 .. c0 + 3; hq[0 .. 4] <- the taps of x, y, x^2, y^2, x y
__device__ __forceinline__ void horizontal_pair(const float (*sx)[HXS], const float (*sy)[HXS], float (*hq)[HY][TX], const Window& win, int tid)
{
    if (tid < HY * (TX / 4)) {
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
}

// horizontal taps of N independent planes: hq[q] <- the taps of sm[q]
template <int N>
__device__ __forceinline__ void horizontal_planes(const float (*sm)[HY][HXS], float (*hq)[HY][TX], const Window& win, int tid)
{
    if (tid < HY * (TX / 4)) {
        const int r = tid >> 3, c0 = (tid & 7) * 4;
#pragma unroll
        for (int q = 0; q < N; ++q) {
            float v[WIN + 3];
#pragma unroll
            for (int k = 0; k < WIN + 3; ++k) v[k] = sm[q][r][c0 + k];
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < WIN; ++k) a += win.w[k] * v[j + k];
                o[j] = a;
            }
            *reinterpret_cast<float4*>(&hq[q][r][c0]) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// vertical taps: thread tid owns column tx = tid & 31 of the tile and its rows ty0 = (tid >> 5) * 2 and ty0 + 1.  load_columns reads the
// WIN + 1 values of each of the M planes that the two rows need; window_sums forms the M windowed sums of row ty0 + j (j = 0, 1).  Two calls
// instead of one that returns both rows: the caller finishes a row before the next one's sums take registers.
template <int M>
__device__ __forceinline__ void load_columns(const float (*hq)[HY][TX], int tx, int ty0, float (&col)[M][WIN + 1])
{
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int k = 0; k < WIN + 1; ++k) col[m][k] = hq[m][ty0 + k][tx];
}
template <int M>
__device__ __forceinline__ void window_sums(const float (&col)[M][WIN + 1], const Window& win, int j, float (&s)[M])
{
#pragma unroll
    for (int m = 0; m < M; ++m) s[m] = 0.f;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
        const float w = win.w[k];
#pragma unroll
        for (int m = 0; m < M; ++m) s[m] += w * col[m][j + k];
    }
}

// the sum of a value over the 256 threads in a fixed order: every wave's DPP sum (wave_reduce::wave_sum_hi, valid in lane 63) goes to
// red[wave]; after the caller's __syncthreads() block_sum(red) is (r0 + r1) + (r2 + r3).  Two steps so that several values share one barrier.
template <typename T>
__device__ __forceinline__ void block_sum_post(T (&red)[4], T wave_sum, int tid)
{
    if ((tid & 63) == 63) red[tid >> 6] = wave_sum;
}
template <typename T>
__device__ __forceinline__ T block_sum(const T (&red)[4])
{
    return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace ssim_window

// gfs_kernels.hip -- the resident frame store (include/gfs.h): the ground truth of a training frame kept in HBM as the 8-bit RGB image it
// is by construction (scene/__init__.py:51 quantises before :54 divides), composited once at ingest and expanded to the planar fp32
// `original_image` by one launch per iteration instead of a 5.3 MB pageable upload.
//
// A frame whose file is not of the camera's size goes through Pillow's bicubic resize on the way in (k_resample_h, k_resample_v: further down).
//
// The first two kernels are streaming passes, a lane per group of four neighbouring pixels:
//   k_compose   16 bytes of RGBA in (one uint4 where the source allows), 12 bytes of RGB out as three dwords.  fp64 throughout; the 256
//               quotients byte / 255.0 are formed once per workgroup into LDS (one IEEE division per thread), the rest is two multiplies, a
//               subtraction, an addition and a multiply per channel in the reference's order.
//   k_fetch     three dwords in, four floats per plane out (one 16-byte store per plane where the planes are 16-byte aligned).  The
//               byte-to-float map is the caller's 256-entry table, staged in LDS: no division here, the floats are torch's.
// A frame's stride covers whole groups of four pixels (gfs_frame_stride), so no load or store of a lane leaves its frame; what is guarded
// is the RGBA source's tail and the planes' tail, which have no such padding.
// Built with -ffp-contract=off: n_rgb * n_a + bg * (1 - n_a) must round as numpy rounds it, product by product.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gfs.h"
#include "launch_prof.h"
#include "lib_common.h"

namespace gfs {

constexpr int BLOCK = 256;
static_assert(BLOCK == GFS_TABLE_ENTRIES, "a workgroup stages the table one entry per thread");

// one channel of scene/__init__.py:50-51: the fp64 composite, times 255, truncated, its low 8 bits
__device__ __forceinline__ unsigned composed(double n, double na, double one_minus_na, double bg)
{
    const double arr = n * na + bg * one_minus_na;
    const double v = arr * 255.0;
    return (unsigned)(int)v & 0xffu;
}

template <bool ALIGNED>
__global__ __launch_bounds__(BLOCK) void k_compose(int HW, int groups, const unsigned char* __restrict__ rgba, double bg0, double bg1, double bg2,
                                                    unsigned char* __restrict__ store, long long stride, long long first)
{
    __shared__ double norm[GFS_TABLE_ENTRIES];
    norm[threadIdx.x] = (double)threadIdx.x / 255.0;
    __syncthreads();
    const int g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= groups) return;
    const long long f = blockIdx.y;
    const unsigned* __restrict__ src = reinterpret_cast<const unsigned*>(rgba + f * (long long)HW * 4);   // (a pixel is one dword)
    const int p = g * 4;
    unsigned px[4];
    if (ALIGNED) {
        const uint4 q = *reinterpret_cast<const uint4*>(src + p);
        px[0] = q.x; px[1] = q.y; px[2] = q.z; px[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j] = p + j < HW ? src[p + j] : 0u;
    }
    unsigned o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double na = norm[px[j] >> 24], rest = 1.0 - na;
        const bool live = ALIGNED || p + j < HW;   // (the padding behind the last pixel: zeros)
        o[3 * j] = live ? composed(norm[px[j] & 0xffu], na, rest, bg0) : 0u;
        o[3 * j + 1] = live ? composed(norm[(px[j] >> 8) & 0xffu], na, rest, bg1) : 0u;
        o[3 * j + 2] = live ? composed(norm[(px[j] >> 16) & 0xffu], na, rest, bg2) : 0u;
    }
    unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(store + (first + f) * stride + (long long)g * 12);
    dst[0] = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    dst[1] = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
    dst[2] = o[8] | (o[9] << 8) | (o[10] << 16) | (o[11] << 24);
}

// blockIdx.y = k, the image of the output; its frame is indices[k] (device) or `host_index` when `indices` is null
template <bool ALIGNED>
__global__ __launch_bounds__(BLOCK) void k_fetch(int HW, int groups, const unsigned char* __restrict__ store, long long stride, long long count,
                                                  const long long* __restrict__ indices, long long host_index, const float* __restrict__ table,
                                                  float* __restrict__ out, int* flag)
{
    __shared__ float lut[GFS_TABLE_ENTRIES];
    const long long k = blockIdx.y;
    const long long frame = indices ? indices[k] : host_index;   // (uniform over the workgroup: all of it leaves, or none)
    if (frame < 0 || frame >= count) {
        if (flag && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(flag, GFS_FLAG_RANGE);
        return;
    }
    lut[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const int g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= groups) return;
    const unsigned* __restrict__ w = reinterpret_cast<const unsigned*>(store + frame * stride + (long long)g * 12);
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
    const float r[4] = {lut[w0 & 0xffu], lut[w0 >> 24], lut[(w1 >> 16) & 0xffu], lut[(w2 >> 8) & 0xffu]};
    const float gr[4] = {lut[(w0 >> 8) & 0xffu], lut[w1 & 0xffu], lut[w1 >> 24], lut[(w2 >> 16) & 0xffu]};
    const float b[4] = {lut[(w0 >> 16) & 0xffu], lut[(w1 >> 8) & 0xffu], lut[w2 & 0xffu], lut[w2 >> 24]};
    const int p = g * 4;
    float* __restrict__ o = out + k * 3 * (long long)HW + p;
    if (ALIGNED) {
        *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(o + HW) = make_float4(gr[0], gr[1], gr[2], gr[3]);
        *reinterpret_cast<float4*>(o + 2 * (long long)HW) = make_float4(b[0], b[1], b[2], b[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p + j < HW) {
                o[j] = r[j];
                o[HW + j] = gr[j];
                o[2 * (long long)HW + j] = b[j];
            }
    }
}

// ---- Pillow's resize of an 8-bit RGB image (include/gfs.h: gfs_resample): two separable passes in 32-bit integers ---------------------------------
// The coefficients are the caller's (host doubles, rounded to 22 fractional bits there); a kernel only multiplies bytes by them, adds in int32
// and shifts.  Both passes keep k_compose's unit of work -- a lane owns a group of four neighbouring pixels of the OUTPUT frame, counted along
// the frame, so its 12 bytes are three aligned dwords whatever the row length is -- and a group may therefore straddle a row end: every pixel
// of a lane has its own (row, column).
constexpr int RS_ROWS = 4;        // row quads a lane of the horizontal pass takes: a coefficient it loads serves RS_ROWS * 3 products
constexpr int RS_SPAN = 15360;    // LDS bytes per row quad of the horizontal pass (RS_ROWS * RS_SPAN = 60 KiB of the 64 KiB a workgroup may declare)

// bounds[2 i], bounds[2 i + 1] = (first tap, taps) of output index i, held to the axis whatever the table says: no read leaves a row or a column
__device__ __forceinline__ void window_of(const int* __restrict__ bounds, int i, int in_size, int ks, int& first, int& taps)
{
    first = min(max(bounds[2 * i], 0), in_size - 1);
    taps = max(min(min(bounds[2 * i + 1], ks), in_size - first), 1);
}

// one product of the sum: a byte times a coefficient of at most 24 bits with its sign (Pillow's stay below 2^23), added in int32: the 24-bit
// multiply-add is exact on these and is one instruction
__device__ __forceinline__ int mac(int acc, unsigned byte, int k) { return acc + __mul24((int)byte, k); }

// clamp(acc >> 22, 0, 255), with the clamp in front of the shift (the same byte: below zero 0, from 256 << 22 on 255).  Written shift-first, pairs
// of these became gfx950's v_ashr_pk_u8_i32, whose upper 16 result bits the compiler ORs into a dword as zeros; on the MI355X they were not,
// and the upper two bytes of a lane's second dword came out wrong while the same source was exact on the host.
__device__ __forceinline__ unsigned to_byte(int acc) { return (unsigned)min(max(acc, 0), (256 << 22) - 1) >> 22; }

__device__ __forceinline__ void store_group(unsigned char* __restrict__ frame, int g, int groups, long long stride, const unsigned (&o)[12])
{
    unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(frame + (long long)g * 12);
    dst[0] = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    dst[1] = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
    dst[2] = o[8] | (o[9] << 8) | (o[10] << 16) | (o[11] << 24);
    if (g == groups - 1)   // (what the stride adds behind the last group: zeros too)
        for (long long b = (long long)groups * 12; b < stride; b += 4) *reinterpret_cast<unsigned*>(frame + b) = 0u;
}

// Horizontal pass: (H, Win) -> (H, Wout).  blockIdx = (256 groups of a row quad, band of 4 * RS_ROWS rows, frame).  A quad of rows is Wout groups
// exactly, so group i of the quads 0 .. RS_ROWS-1 of a band are the same four columns, four rows further down each: the lane loads the
// coefficient of a tap once per column and uses it on RS_ROWS rows.  The source bytes a workgroup's pixels read are one contiguous piece of the
// frame per quad (windows only move forward along a row, rows follow each other); it is staged in LDS with 16-byte loads when it fits
// RS_SPAN -- down-scales to about a fifth -- and read from global memory otherwise.
template <bool STAGED>
__device__ __forceinline__ void taps_h(const unsigned char* __restrict__ in, const unsigned char (*seg)[RS_SPAN], const int (&rowbase)[RS_ROWS],
                                       const int (&segbase)[RS_ROWS], const int* const (&kr)[4], const int (&idx0)[4], const int (&n)[4],
                                       const bool (&live)[RS_ROWS][4], int (&acc)[RS_ROWS][4][3])
{
    const int nmax = max(max(n[0], n[1]), max(n[2], n[3]));
    for (int t = 0; t < nmax; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = t < n[j] ? kr[j][t] : 0;
            const int at = idx0[j] + min(t, n[j] - 1) * 3;
#pragma unroll
            for (int k = 0; k < RS_ROWS; ++k) {
                if (!live[k][j]) continue;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    acc[k][j][ch] = mac(acc[k][j][ch], STAGED ? seg[k][at + ch + segbase[k]] : in[rowbase[k] + at + ch], c);
                }
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_resample_h(int H, int Win, int Wout, const unsigned char* __restrict__ src, long long src_stride,
                                                       const int* __restrict__ kx, const int* __restrict__ bx, int ks,
                                                       unsigned char* __restrict__ dst, long long dst_stride)
{
    __shared__ __attribute__((aligned(16))) unsigned char seg[RS_ROWS][RS_SPAN];
    const unsigned char* __restrict__ in = src + (long long)blockIdx.z * src_stride;
    const int in_bytes = H * Win * 3, groups = (H * Wout + 3) / 4;
    const int band_row = blockIdx.y * 4 * RS_ROWS;
    // the piece of a row quad this workgroup reads, in bytes from the quad's first row: [s, e)
    const int r_first = blockIdx.x * BLOCK * 4, r_last = min(r_first + BLOCK * 4, 4 * Wout) - 1;
    int first, taps;
    window_of(bx, r_first % Wout, Win, ks, first, taps);
    const int s = ((r_first / Wout) * Win + first) * 3;
    window_of(bx, r_last % Wout, Win, ks, first, taps);
    const int e = ((r_last / Wout) * Win + first + taps) * 3;
    const bool staged = e - s + 30 <= RS_SPAN;   // (up to 15 bytes in front for the alignment, up to 15 behind for the last 16-byte load)
    int rowbase[RS_ROWS], segbase[RS_ROWS];
#pragma unroll
    for (int k = 0; k < RS_ROWS; ++k) {
        rowbase[k] = (band_row + 4 * k) * Win * 3;   // (rows past the frame: no pixel of theirs is live, nothing is read)
        const int a0 = (rowbase[k] + s) & ~15, end = min(rowbase[k] + e, in_bytes);
        segbase[k] = rowbase[k] - a0;
        if (staged && band_row + 4 * k < H)
            for (int o = threadIdx.x * 16; a0 + o < end; o += BLOCK * 16)   // (a0 + o + 16 <= the stride: both are multiples of 16)
                *reinterpret_cast<uint4*>(&seg[k][o]) = *reinterpret_cast<const uint4*>(in + a0 + o);
    }
    __syncthreads();
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= Wout) return;
    const int* kr[4];
    int idx0[4], n[4], acc[RS_ROWS][4][3];
    bool live[RS_ROWS][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 4 * i + j, yr = r / Wout, x = r - yr * Wout;
        window_of(bx, x, Win, ks, first, n[j]);
        kr[j] = kx + (long long)x * ks;
        idx0[j] = (yr * Win + first) * 3;
#pragma unroll
        for (int k = 0; k < RS_ROWS; ++k) {
            live[k][j] = band_row + 4 * k + yr < H;
            acc[k][j][0] = acc[k][j][1] = acc[k][j][2] = 1 << 21;
        }
    }
    if (staged) taps_h<true>(in, seg, rowbase, segbase, kr, idx0, n, live, acc);
    else taps_h<false>(in, seg, rowbase, segbase, kr, idx0, n, live, acc);
    unsigned char* __restrict__ out = dst + (long long)blockIdx.z * dst_stride;
#pragma unroll
    for (int k = 0; k < RS_ROWS; ++k) {
        const int g = (band_row / 4 + k) * Wout + i;
        if (g >= groups) break;
        unsigned o[12];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[3 * j + ch] = live[k][j] ? to_byte(acc[k][j][ch]) : 0u;
        store_group(out, g, groups, dst_stride, o);
    }
}

// Vertical pass: (Hin, W) -> (Hout, W).  blockIdx = (256 groups of the output frame, frame); lanes run along the row, so a tap's loads of a wave
// are one piece of a source row.  A group inside one row reads its 12 bytes of a tap as the four aligned dwords around them, shifted into
// place; a group across a row end reads bytes.  The coefficient of a tap is one load per 12 products.
__global__ __launch_bounds__(BLOCK) void k_resample_v(int Hin, int Hout, int W, const unsigned char* __restrict__ src, long long src_stride,
                                                       const int* __restrict__ ky, const int* __restrict__ by, int ks,
                                                       unsigned char* __restrict__ dst, long long dst_stride)
{
    const int HW = Hout * W, groups = (HW + 3) / 4;
    const int g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= groups) return;
    const unsigned char* __restrict__ in = src + (long long)blockIdx.y * src_stride;
    const int p = g * 4, y0 = p / W, x0 = p - y0 * W, row = W * 3;
    unsigned o[12];
    if (x0 + 3 < W) {   // (one row; then p + 3 < HW too)
        int first, n, acc[12];
        window_of(by, y0, Hin, ks, first, n);
        const int* __restrict__ kr = ky + (long long)y0 * ks;
#pragma unroll
        for (int b = 0; b < 12; ++b) acc[b] = 1 << 21;
        int a = (first * W + x0) * 3;
        for (int t = 0; t < n; ++t, a += row) {
            const int c = kr[t], sh = a & 3;
            const unsigned* __restrict__ w = reinterpret_cast<const unsigned*>(in + (a - sh));
            const unsigned d0 = w[0], d1 = w[1], d2 = w[2], d3 = sh ? w[3] : 0u;   // (a + 11 is inside the frame, so w[3] is inside its stride when sh > 0)
            const unsigned v[3] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh), __builtin_amdgcn_alignbyte(d3, d2, sh)};
#pragma unroll
            for (int b = 0; b < 12; ++b) acc[b] = mac(acc[b], (v[b >> 2] >> (8 * (b & 3))) & 0xffu, c);
        }
#pragma unroll
        for (int b = 0; b < 12; ++b) o[b] = to_byte(acc[b]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = 0u;   // (the padding behind the last pixel: zeros)
            if (p + j >= HW) continue;
            const int y = (p + j) / W, x = p + j - y * W;
            int first, n, acc[3] = {1 << 21, 1 << 21, 1 << 21};
            window_of(by, y, Hin, ks, first, n);
            const int* __restrict__ kr = ky + (long long)y * ks;
            int a = (first * W + x) * 3;
            for (int t = 0; t < n; ++t, a += row) {
                const int c = kr[t];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] = mac(acc[ch], in[a + ch], c);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[3 * j + ch] = to_byte(acc[ch]);
        }
    }
    store_group(dst + (long long)blockIdx.y * dst_stride, g, groups, dst_stride, o);
}

}  // namespace gfs

// ---------------------------------------------------------------------------------------------------------------
static bool shape_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W <= (int64_t)INT32_MAX / 4; }

static int64_t stride_of(int64_t HW) { return (((HW + 3) / 4) * 12 + 15) / 16 * 16; }

static int fetch_impl(int32_t H, int32_t W, const uint8_t* store, int64_t count, const int64_t* indices, int64_t host_index, int32_t K,
                      const float* table, float* out, int32_t* flag, void* stream_)
{
    if (!shape_ok(H, W)) return fail(GFS_E_ARG, "bad image shape (%d,%d)", H, W);
    if (!store || !table || !out) return fail(GFS_E_ARG, "null pointer");
    if (count <= 0) return fail(GFS_E_ARG, "count must be positive (got %lld)", (long long)count);
    if (K <= 0 || K > GFS_MAX_BATCH) return fail(GFS_E_ARG, "K must be in [1, %d] (got %d)", GFS_MAX_BATCH, K);
    if ((uintptr_t)store & 15) return fail(GFS_E_ARG, "the store must be 16-byte aligned");
    if (((uintptr_t)table | (uintptr_t)out | (uintptr_t)flag) & 3) return fail(GFS_E_ARG, "table, out and flag must be 4-byte aligned");
    if ((uintptr_t)indices & 7) return fail(GFS_E_ARG, "indices must be 8-byte aligned");
    if (!indices && (host_index < 0 || host_index >= count))
        return fail(GFS_E_RANGE, "frame index %lld outside [0, %lld)", (long long)host_index, (long long)count);
    const int HW = H * W, groups = (HW + 3) / 4;
    const dim3 grid((unsigned)((groups + gfs::BLOCK - 1) / gfs::BLOCK), (unsigned)K);
    hipStream_t stream = (hipStream_t)stream_;
    if ((HW & 3) == 0 && !((uintptr_t)out & 15)) {
        PROF_LAUNCH(gfs::k_fetch<true>, grid, dim3(gfs::BLOCK), 0, stream, HW, groups, store, (long long)stride_of(HW), (long long)count,
                    (const long long*)indices, (long long)host_index, table, out, (int*)flag);
    } else {
        PROF_LAUNCH(gfs::k_fetch<false>, grid, dim3(gfs::BLOCK), 0, stream, HW, groups, store, (long long)stride_of(HW), (long long)count,
                    (const long long*)indices, (long long)host_index, table, out, (int*)flag);
    }
    LAUNCH_CHECK(GFS_E_HIP, "k_fetch");
    return GFS_OK;
}

extern "C" {

int gfs_abi_version(void) { return GFS_ABI_VERSION; }
const char* gfs_last_error(void) { return g_err; }

int64_t gfs_frame_stride(int32_t H, int32_t W) { return shape_ok(H, W) ? stride_of((int64_t)H * W) : 0; }

int gfs_compose(int32_t H, int32_t W, const uint8_t* rgba, const double* bg, uint8_t* store, int64_t capacity, int64_t first, int32_t count,
                void* stream_)
{
    if (!shape_ok(H, W)) return fail(GFS_E_ARG, "bad image shape (%d,%d)", H, W);
    if (!rgba || !bg || !store) return fail(GFS_E_ARG, "null pointer");
    if (count <= 0 || count > GFS_MAX_BATCH) return fail(GFS_E_ARG, "count must be in [1, %d] (got %d)", GFS_MAX_BATCH, count);
    if (first < 0 || capacity <= 0 || first > capacity - count)
        return fail(GFS_E_RANGE, "frames [%lld, %lld) outside a store of %lld", (long long)first, (long long)first + count, (long long)capacity);
    if ((uintptr_t)store & 15) return fail(GFS_E_ARG, "the store must be 16-byte aligned");
    if ((uintptr_t)rgba & 3) return fail(GFS_E_ARG, "rgba must be 4-byte aligned");
    const int HW = H * W, groups = (HW + 3) / 4;
    const dim3 grid((unsigned)((groups + gfs::BLOCK - 1) / gfs::BLOCK), (unsigned)count);
    hipStream_t stream = (hipStream_t)stream_;
    if ((HW & 3) == 0 && !((uintptr_t)rgba & 15)) {
        PROF_LAUNCH(gfs::k_compose<true>, grid, dim3(gfs::BLOCK), 0, stream, HW, groups, rgba, bg[0], bg[1], bg[2], store, (long long)stride_of(HW),
                    (long long)first);
    } else {
        PROF_LAUNCH(gfs::k_compose<false>, grid, dim3(gfs::BLOCK), 0, stream, HW, groups, rgba, bg[0], bg[1], bg[2], store, (long long)stride_of(HW),
                    (long long)first);
    }
    LAUNCH_CHECK(GFS_E_HIP, "k_compose");
    return GFS_OK;
}

int64_t gfs_resample_tmp_bytes(int32_t Hin, int32_t Wout, int32_t count)
{
    return shape_ok(Hin, Wout) && count > 0 && count <= GFS_MAX_BATCH ? stride_of((int64_t)Hin * Wout) * count : 0;
}

int gfs_resample(int32_t Hin, int32_t Win, const uint8_t* src, int64_t src_capacity, int64_t src_first, int32_t Hout, int32_t Wout,
                 const int32_t* kx, const int32_t* bx, int32_t ksx, const int32_t* ky, const int32_t* by, int32_t ksy, uint8_t* tmp, uint8_t* store,
                 int64_t capacity, int64_t first, int32_t count, void* stream_)
{
    if (!shape_ok(Hin, Win) || !shape_ok(Hout, Wout) || !shape_ok(Hin, Wout))
        return fail(GFS_E_ARG, "bad image shape (%d,%d) -> (%d,%d)", Hin, Win, Hout, Wout);
    const bool horizontal = Win != Wout, vertical = Hin != Hout;
    if (!horizontal && !vertical) return fail(GFS_E_ARG, "nothing to resample: (%d,%d) is the size of the source", Hout, Wout);
    if (!src || !store) return fail(GFS_E_ARG, "null pointer");
    if (horizontal != (kx != nullptr) || horizontal != (bx != nullptr) || vertical != (ky != nullptr) || vertical != (by != nullptr))
        return fail(GFS_E_ARG, "the tables of an axis must be given when its size changes and be null when it does not");
    if (horizontal && vertical && !tmp) return fail(GFS_E_ARG, "null pointer (tmp: both axes change)");
    if ((horizontal && ksx < 1) || (vertical && ksy < 1)) return fail(GFS_E_ARG, "ksize must be positive (got %d, %d)", ksx, ksy);
    if (count <= 0 || count > GFS_MAX_BATCH) return fail(GFS_E_ARG, "count must be in [1, %d] (got %d)", GFS_MAX_BATCH, count);
    if (src_first < 0 || src_capacity <= 0 || src_first > src_capacity - count)
        return fail(GFS_E_RANGE, "source frames [%lld, %lld) outside a store of %lld", (long long)src_first, (long long)src_first + count,
                    (long long)src_capacity);
    if (first < 0 || capacity <= 0 || first > capacity - count)
        return fail(GFS_E_RANGE, "frames [%lld, %lld) outside a store of %lld", (long long)first, (long long)first + count, (long long)capacity);
    if (((uintptr_t)src | (uintptr_t)store | (uintptr_t)tmp) & 15) return fail(GFS_E_ARG, "the stores and tmp must be 16-byte aligned");
    if (((uintptr_t)kx | (uintptr_t)bx | (uintptr_t)ky | (uintptr_t)by) & 3) return fail(GFS_E_ARG, "the tables must be 4-byte aligned");
    const int bands = (Hin + 4 * gfs::RS_ROWS - 1) / (4 * gfs::RS_ROWS);
    if (horizontal && bands > 65535) return fail(GFS_E_ARG, "bad image shape (%d,%d): more than %d rows", Hin, Win, 65535 * 4 * gfs::RS_ROWS);
    hipStream_t stream = (hipStream_t)stream_;
    const long long s_in = stride_of((int64_t)Hin * Win), s_mid = stride_of((int64_t)Hin * Wout), s_out = stride_of((int64_t)Hout * Wout);
    const uint8_t* from = src + src_first * s_in;
    uint8_t* to = store + first * s_out;
    if (horizontal) {   // Pillow's order: the horizontal axis first, bytes in between
        const dim3 grid((unsigned)((Wout + gfs::BLOCK - 1) / gfs::BLOCK), (unsigned)bands, (unsigned)count);
        PROF_LAUNCH(gfs::k_resample_h, grid, dim3(gfs::BLOCK), 0, stream, Hin, Win, Wout, from, s_in, kx, bx, ksx, vertical ? tmp : to,
                    vertical ? s_mid : s_out);
        LAUNCH_CHECK(GFS_E_HIP, "k_resample_h");
    }
    if (vertical) {
        const int groups = (Hout * Wout + 3) / 4;
        const dim3 grid((unsigned)((groups + gfs::BLOCK - 1) / gfs::BLOCK), (unsigned)count);
        PROF_LAUNCH(gfs::k_resample_v, grid, dim3(gfs::BLOCK), 0, stream, Hin, Hout, Wout, horizontal ? (const uint8_t*)tmp : from,
                    horizontal ? s_mid : s_in, ky, by, ksy, to, s_out);
        LAUNCH_CHECK(GFS_E_HIP, "k_resample_v");
    }
    return GFS_OK;
}

int gfs_fetch(int32_t H, int32_t W, const uint8_t* store, int64_t count, int64_t index, const float* table, float* out, void* stream)
{
    return fetch_impl(H, W, store, count, nullptr, index, 1, table, out, nullptr, stream);
}

int gfs_fetch_indexed(int32_t H, int32_t W, const uint8_t* store, int64_t count, const int64_t* index, const float* table, float* out,
                      int32_t* flag, void* stream)
{
    if (!index || !flag) return fail(GFS_E_ARG, "null pointer");
    return fetch_impl(H, W, store, count, index, 0, 1, table, out, flag, stream);
}

int gfs_fetch_batch(int32_t H, int32_t W, const uint8_t* store, int64_t count, const int64_t* indices, int32_t K, const float* table, float* out,
                    int32_t* flag, void* stream)
{
    if (!indices || !flag) return fail(GFS_E_ARG, "null pointer");
    return fetch_impl(H, W, store, count, indices, 0, K, table, out, flag, stream);
}

LPROF_EXPORTS(gfs)

}  // extern "C"

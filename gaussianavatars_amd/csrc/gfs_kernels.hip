// gfs_kernels.hip -- the resident frame store (include/gfs.h): the ground truth of a training frame kept in HBM as the 8-bit RGB image it
// is by construction (scene/__init__.py:51 quantises before :54 divides), composited once at ingest and expanded to the planar fp32
// `original_image` by one launch per iteration instead of a 5.3 MB pageable upload.
//
// Both kernels are streaming passes, a lane per group of four neighbouring pixels:
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

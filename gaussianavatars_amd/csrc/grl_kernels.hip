// grl_kernels.hip -- the fused splat regularisers of include/grl.h: train.py:134-146 in one launch forward and one launch backward.
//
// Launch shape (both kernels): one 256-thread workgroup per GRL_SLAB (1024) splats, FOUR CONSECUTIVE splats per lane.  Four 12-byte rows are
// 48 bytes: a lane reads its rows of `xyz` and of `log_scaling` with three 16-byte loads each and its four `visible` bytes with one 4-byte
// load -- all seven issued before the first use, 100 B per lane and 25 KiB per workgroup in flight -- where one lane per splat would have
// issued one round of 4-byte loads.  The workgroup of the array's last, partial slab, and every workgroup when a base pointer is not 16-byte
// aligned (a row-sliced view), takes the element-wise loads of the same code: the choice is per workgroup, a scalar branch.  The backward
// stores the same way.
//
// Forward reduction: lanes add their (at most four) visible terms in splat order, a workgroup reduces in a fixed shuffle / LDS tree and lane 0
// publishes one partial {sum a, sum b, count} per workgroup, then draws an arrival ticket (the ONE integer atomic of the workgroup).  The
// workgroup that draws the last ticket sums the partials in double -- lane t takes workgroups t, t + 256, ..., then the same fixed tree --
// writes `out` and resets the arrival word.  The hand-off is the agent-scope one: partials are stored write-through (relaxed agent-scope
// atomic stores), drained, released; the last arriver acquires and reads them with agent-scope loads, so the result does not depend on which
// XCD a workgroup ran on.  Partials are plain floats: a NaN or Inf in a visible row reaches the mean.  No float atomics anywhere.
//
// Compiled with -ffp-contract=off: the roundings per splat are the ones grl.h lists, whatever the compiler version, and the forward's a_i / b_i
// are bit for bit the values whose sign the backward's masks test (the backward recomputes them: a contraction in one of the two kernels
// only could put a splat above the threshold in one pass and at it in the other).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/grl.h"
#include "launch_prof.h"
#include "lib_common.h"

namespace grl {

constexpr int BLOCK = 256;
constexpr int PER = 4;   // consecutive splats per lane
constexpr int SLAB = GRL_SLAB;
constexpr int WAVES = BLOCK / 64;
static_assert(SLAB == BLOCK * PER, "a slab is four splats per lane");
constexpr int SCRATCH_HEAD = 16;      // bytes: the arrival word, in a 16-byte block of its own at the start of the scratch
constexpr int PARTIAL_FLOATS = 4;     // {sum a, sum b, count, unused} per workgroup

typedef float v4f __attribute__((ext_vector_type(4)));   // (stores through HIP's float4 struct came out as 12-byte pieces)

__device__ __forceinline__ float relu(float d) { return d <= 0.f ? 0.f : d; }   // (a NaN stays a NaN)

// the lane's four rows of a (P,3) array, first row i0, `nvalid` of them inside the array; rows past the end read as 0.
// VEC (chosen per WORKGROUP, so the branch is uniform: aligned bases and a whole slab inside the array) is the 16-byte form.
template <bool VEC>
__device__ __forceinline__ void load_rows(const float* __restrict__ p, long long i0, int nvalid, float (&r)[3 * PER])
{
    if (VEC) {
        const float4* q = reinterpret_cast<const float4*>(p + 3 * i0);   // i0 is a multiple of 4: 48-byte steps from a 16-byte aligned base
        const float4 a = q[0], b = q[1], c = q[2];
        r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w, r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w, r[8] = c.x, r[9] = c.y, r[10] = c.z, r[11] = c.w;
    } else {
#pragma unroll
        for (int j = 0; j < 3 * PER; ++j) r[j] = j < 3 * nvalid ? p[3 * i0 + j] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_rows(float* __restrict__ p, long long i0, int nvalid, const float (&r)[3 * PER])
{
    if (VEC) {
        v4f* q = reinterpret_cast<v4f*>(p + 3 * i0);
        q[0] = v4f{r[0], r[1], r[2], r[3]};
        q[1] = v4f{r[4], r[5], r[6], r[7]};
        q[2] = v4f{r[8], r[9], r[10], r[11]};
    } else {
#pragma unroll
        for (int j = 0; j < 3 * PER; ++j)
            if (j < 3 * nvalid) p[3 * i0 + j] = r[j];
    }
}

// bit k set: splat i0 + k is inside the array and visible
template <bool VEC>
__device__ __forceinline__ unsigned load_visible(const unsigned char* __restrict__ v, long long i0, int nvalid)
{
    unsigned m = 0;
    if (VEC) {
        const unsigned w = *reinterpret_cast<const unsigned*>(v + i0);
#pragma unroll
        for (int k = 0; k < PER; ++k) m |= ((w >> (8 * k)) & 0xffu) ? (1u << k) : 0u;
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (k < nvalid && v[i0 + k]) m |= 1u << k;
    }
    return m;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T x)   // fixed tree: lane 0 holds the sum of the wave's 64 values
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

template <bool ALIGNED>
__global__ __launch_bounds__(BLOCK) void k_reg_fwd(int P, const float* __restrict__ xyz, const float* __restrict__ ls, const unsigned char* __restrict__ vis,
                                                   float t_xyz, float t_s, float* out, unsigned* arrival, float* partials)
{
    __shared__ double sh[3 * WAVES + 1];   // (the one LDS object: wave partials, then the "I am last" word)
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = (int)blockIdx.x, nwg = (int)gridDim.x;
    const long long i0 = (long long)wg * SLAB + (long long)tid * PER;
    const long long left = (long long)P - i0;
    const int nvalid = left >= PER ? PER : (left > 0 ? (int)left : 0);

    const bool vec = ALIGNED && (long long)(wg + 1) * SLAB <= (long long)P;   // workgroup-uniform

    float X[3 * PER], S[3 * PER];
    unsigned m;
    if (vec) {
        load_rows<true>(xyz, i0, nvalid, X);
        load_rows<true>(ls, i0, nvalid, S);
        m = load_visible<true>(vis, i0, nvalid);
    } else {
        load_rows<false>(xyz, i0, nvalid, X);
        load_rows<false>(ls, i0, nvalid, S);
        m = load_visible<false>(vis, i0, nvalid);
    }

    float sa = 0.f, sb = 0.f, cnt = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const float x = X[3 * k], y = X[3 * k + 1], z = X[3 * k + 2];
        const float a = relu(sqrtf(x * x + y * y + z * z) - t_xyz);
        const float v0 = relu(expf(S[3 * k]) - t_s), v1 = relu(expf(S[3 * k + 1]) - t_s), v2 = relu(expf(S[3 * k + 2]) - t_s);
        const float b = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
        if (m & (1u << k)) sa += a, sb += b, cnt += 1.f;   // (an invisible row is never added, whatever it holds)
    }
    sa = wave_sum(sa), sb = wave_sum(sb), cnt = wave_sum(cnt);
    if (lane == 0) sh[3 * wave] = (double)sa, sh[3 * wave + 1] = (double)sb, sh[3 * wave + 2] = (double)cnt;
    __syncthreads();
    if (tid == 0) {
        float pa = (float)sh[0], pb = (float)sh[1], pc = (float)sh[2];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) pa += (float)sh[3 * w], pb += (float)sh[3 * w + 1], pc += (float)sh[3 * w + 2];
        float* mine = partials + (long long)wg * PARTIAL_FLOATS;
        __hip_atomic_store(mine + 0, pa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through stores ...
        __hip_atomic_store(mine + 1, pb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + 2, pc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                 // ... drained ...
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                               // ... and released before the ticket is drawn
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(arrival, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = ticket == (unsigned)(nwg - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        sh[3 * WAVES] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    if (sh[3 * WAVES] == 0.0) return;   // workgroup-uniform

    // the last arriver: every partial, in double, in a fixed order
    double da = 0.0, db = 0.0, dc = 0.0;
    for (int w = tid; w < nwg; w += BLOCK) {
        const float* q = partials + (long long)w * PARTIAL_FLOATS;
        da += (double)__hip_atomic_load(q + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        db += (double)__hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dc += (double)__hip_atomic_load(q + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    da = wave_sum(da), db = wave_sum(db), dc = wave_sum(dc);
    __syncthreads();   // (sh[3 * WAVES] has been read by everybody; the wave slots are free again)
    if (lane == 0) sh[3 * wave] = da, sh[3 * wave + 1] = db, sh[3 * wave + 2] = dc;
    __syncthreads();
    if (tid == 0) {
        double ta = sh[0], tb = sh[1], tc = sh[2];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) ta += sh[3 * w], tb += sh[3 * w + 1], tc += sh[3 * w + 2];
        out[0] = (float)(ta / tc);   // (tc == 0: 0 / 0 = NaN, the mean of an empty tensor)
        out[1] = (float)(tb / tc);
        out[2] = (float)tc;
        out[3] = 0.f;
        __hip_atomic_store(arrival, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call, whatever the data held
    }
}

template <bool ALIGNED>
__global__ __launch_bounds__(BLOCK) void k_reg_bwd(int P, const float* __restrict__ xyz, const float* __restrict__ ls, const unsigned char* __restrict__ vis,
                                                   float t_xyz, float t_s, const float* __restrict__ out, const float* __restrict__ g_xyz,
                                                   const float* __restrict__ g_s, float* __restrict__ d_xyz, float* __restrict__ d_ls)
{
    const int tid = (int)threadIdx.x;
    const long long i0 = (long long)blockIdx.x * SLAB + (long long)tid * PER;
    const long long left = (long long)P - i0;
    const int nvalid = left >= PER ? PER : (left > 0 ? (int)left : 0);
    if (nvalid == 0) return;

    const float c = out[2];
    const bool any = c > 0.f;                       // (c == 0: every gradient is +0, 1 / c is never formed)
    const bool do_x = d_xyz != nullptr, do_s = d_ls != nullptr;
    const bool live_x = do_x && g_xyz != nullptr && any, live_s = do_s && g_s != nullptr && any;
    const float kx = live_x ? g_xyz[0] / c : 0.f, ks = live_s ? g_s[0] / c : 0.f;

    const bool vec = ALIGNED && (long long)(blockIdx.x + 1) * SLAB <= (long long)P;   // workgroup-uniform, as live_x / live_s

    float X[3 * PER], S[3 * PER];
    unsigned m = 0u;
    if (vec) {
        if (live_x) load_rows<true>(xyz, i0, nvalid, X);
        if (live_s) load_rows<true>(ls, i0, nvalid, S);
        if (live_x || live_s) m = load_visible<true>(vis, i0, nvalid);
    } else {
        if (live_x) load_rows<false>(xyz, i0, nvalid, X);
        if (live_s) load_rows<false>(ls, i0, nvalid, S);
        if (live_x || live_s) m = load_visible<false>(vis, i0, nvalid);
    }

    if (do_x) {
        float D[3 * PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            float dx = 0.f, dy = 0.f, dz = 0.f;
            if (live_x && (m & (1u << k))) {
                const float x = X[3 * k], y = X[3 * k + 1], z = X[3 * k + 2];
                const float n = sqrtf(x * x + y * y + z * z);
                if (n - t_xyz > 0.f) dx = kx * (x / n), dy = kx * (y / n), dz = kx * (z / n);
            }
            D[3 * k] = dx, D[3 * k + 1] = dy, D[3 * k + 2] = dz;
        }
        if (vec) store_rows<true>(d_xyz, i0, nvalid, D);
        else store_rows<false>(d_xyz, i0, nvalid, D);
    }
    if (do_s) {
        float D[3 * PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            float d0 = 0.f, d1 = 0.f, d2 = 0.f;
            if (live_s && (m & (1u << k))) {
                const float e0 = expf(S[3 * k]), e1 = expf(S[3 * k + 1]), e2 = expf(S[3 * k + 2]);
                const float v0 = relu(e0 - t_s), v1 = relu(e1 - t_s), v2 = relu(e2 - t_s);
                const float b = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
                if (v0 > 0.f) d0 = (ks * (v0 / b)) * e0;
                if (v1 > 0.f) d1 = (ks * (v1 / b)) * e1;
                if (v2 > 0.f) d2 = (ks * (v2 / b)) * e2;
            }
            D[3 * k] = d0, D[3 * k + 1] = d1, D[3 * k + 2] = d2;
        }
        if (vec) store_rows<true>(d_ls, i0, nvalid, D);
        else store_rows<false>(d_ls, i0, nvalid, D);
    }
}

}  // namespace grl

// ---------------------------------------------------------------------------------------------------------------
static inline bool aligned_to(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
static inline int64_t workgroups(int32_t P) { return P > 0 ? ((int64_t)P + grl::SLAB - 1) / grl::SLAB : 1; }

extern "C" {

int grl_abi_version(void) { return GRL_ABI_VERSION; }
const char* grl_last_error(void) { return g_err; }

int64_t grl_scratch_bytes(int32_t P)
{
    if (P < 0) return fail(GRL_E_ARG, "bad arguments: P < 0");
    if (P >= GRL_MAX_SPLATS) return fail(GRL_E_ARG, "bad arguments: P >= 2^24 (the count would not be an exact float)");
    return (int64_t)grl::SCRATCH_HEAD + workgroups(P) * grl::PARTIAL_FLOATS * (int64_t)sizeof(float);
}

int grl_forward(int32_t P, const void* xyz, const void* log_scaling, const void* visible, float threshold_xyz, float threshold_scale, void* out,
                void* scratch, void* stream_)
{
    if (P < 0) return fail(GRL_E_ARG, "bad arguments: P < 0");
    if (P >= GRL_MAX_SPLATS) return fail(GRL_E_ARG, "bad arguments: P >= 2^24 (the count would not be an exact float)");
    if (!out) return fail(GRL_E_ARG, "bad arguments: NULL out");
    if (!aligned_to(out, 4)) return fail(GRL_E_ARG, "bad arguments: out must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    if (P == 0) {   // no kernel: {NaN, NaN, 0, 0} by two fills on the stream
        hipError_t e = hipMemsetD32Async((hipDeviceptr_t)out, 0x7fc00000, 2, stream);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)((char*)out + 8), 0, 2, stream);
        if (e != hipSuccess) return fail(GRL_E_HIP, "grl_forward (P == 0): %s", hipGetErrorString(e));
        return GRL_OK;
    }
    if (!xyz || !log_scaling || !visible || !scratch) return fail(GRL_E_ARG, "bad arguments: NULL xyz, log_scaling, visible or scratch");
    if (!aligned_to(xyz, 4) || !aligned_to(log_scaling, 4) || !aligned_to(scratch, 16))
        return fail(GRL_E_ARG, "bad arguments: xyz and log_scaling must be 4-byte aligned, scratch 16-byte aligned");
    unsigned* arrival = (unsigned*)scratch;
    float* partials = (float*)((char*)scratch + grl::SCRATCH_HEAD);
    const dim3 grid((unsigned)workgroups(P)), block(grl::BLOCK);
    const bool vec = aligned_to(xyz, 16) && aligned_to(log_scaling, 16) && aligned_to(visible, 4);
    if (vec)
        PROF_LAUNCH(grl::k_reg_fwd<true>, grid, block, 0, stream, (int)P, (const float*)xyz, (const float*)log_scaling, (const unsigned char*)visible,
                    threshold_xyz, threshold_scale, (float*)out, arrival, partials);
    else
        PROF_LAUNCH(grl::k_reg_fwd<false>, grid, block, 0, stream, (int)P, (const float*)xyz, (const float*)log_scaling, (const unsigned char*)visible,
                    threshold_xyz, threshold_scale, (float*)out, arrival, partials);
    LAUNCH_CHECK(GRL_E_HIP, "k_reg_fwd");
    return GRL_OK;
}

int grl_backward(int32_t P, const void* xyz, const void* log_scaling, const void* visible, float threshold_xyz, float threshold_scale, const void* out,
                 const void* g_xyz, const void* g_scale, void* d_xyz, void* d_log_scaling, void* stream_)
{
    if (P < 0) return fail(GRL_E_ARG, "bad arguments: P < 0");
    if (P >= GRL_MAX_SPLATS) return fail(GRL_E_ARG, "bad arguments: P >= 2^24 (the count would not be an exact float)");
    if (P == 0 || (!d_xyz && !d_log_scaling)) return GRL_OK;   // nothing to write
    if (!out || !visible) return fail(GRL_E_ARG, "bad arguments: NULL out or visible");
    if (d_xyz && !xyz) return fail(GRL_E_ARG, "bad arguments: d_xyz wanted with NULL xyz");
    if (d_log_scaling && !log_scaling) return fail(GRL_E_ARG, "bad arguments: d_log_scaling wanted with NULL log_scaling");
    const void* four[] = {out, g_xyz, g_scale, d_xyz ? xyz : nullptr, d_log_scaling ? log_scaling : nullptr, d_xyz, d_log_scaling};
    for (const void* p : four)
        if (!aligned_to(p, 4)) return fail(GRL_E_ARG, "bad arguments: every float pointer must be 4-byte aligned");
    const bool vec = aligned_to(visible, 4) && (!d_xyz || (aligned_to(xyz, 16) && aligned_to(d_xyz, 16))) &&
                     (!d_log_scaling || (aligned_to(log_scaling, 16) && aligned_to(d_log_scaling, 16)));
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)workgroups(P)), block(grl::BLOCK);
    if (vec)
        PROF_LAUNCH(grl::k_reg_bwd<true>, grid, block, 0, stream, (int)P, (const float*)xyz, (const float*)log_scaling, (const unsigned char*)visible,
                    threshold_xyz, threshold_scale, (const float*)out, (const float*)g_xyz, (const float*)g_scale, (float*)d_xyz, (float*)d_log_scaling);
    else
        PROF_LAUNCH(grl::k_reg_bwd<false>, grid, block, 0, stream, (int)P, (const float*)xyz, (const float*)log_scaling, (const unsigned char*)visible,
                    threshold_xyz, threshold_scale, (const float*)out, (const float*)g_xyz, (const float*)g_scale, (float*)d_xyz, (float*)d_log_scaling);
    LAUNCH_CHECK(GRL_E_HIP, "k_reg_bwd");
    return GRL_OK;
}

LPROF_EXPORTS(grl)

}  // extern "C"

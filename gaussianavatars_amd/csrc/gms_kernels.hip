// gms_kernels.hip -- the fused metric-space splat regularisers of include/gms.h: train.py:136 and :143 in one launch forward, one launch
// backward, and one more backward launch for the gradient into face_scaling.
//
// Launch shape (k_metric_fwd, k_metric_bwd), as grl_kernels.hip: one 256-thread workgroup per GMS_SLAB (1024) splats, FOUR CONSECUTIVE
// splats per lane.  Four 12-byte rows are 48 bytes: a lane reads its rows of `xyz` and of `log_scaling` with three 16-byte loads each, its
// four binding indices with one (int32) or two (int64) 16-byte loads and its four `visible` bytes with one 4-byte load, all issued before
// the first use.  The workgroup of the array's last, partial slab, and every workgroup when a base pointer is not 16-byte aligned (a
// row-sliced view), takes the element-wise loads of the same code: the choice is per workgroup, a scalar branch.  The backward stores the
// same way.  face_scaling[binding] is a 4-byte gather per splat from a table of F floats (40 KB at F = 10 144: it stays in L2) and is not
// staged in LDS.  A term that is off (a NULL pointer) issues no load and no arithmetic: the branches on it are scalar.
//
// Forward reduction: the scheme of k_reg_fwd (grl_kernels.hip) with the sums carried in double from the first addition -- lanes add their
// (at most four) visible terms in splat order, a workgroup reduces in a fixed shuffle / LDS tree, lane 0 publishes one partial
// {sum m, sum b, count} and draws an arrival ticket (the ONE integer atomic of the workgroup); the workgroup that draws the last ticket
// sums the partials -- lane t takes workgroups t, t + 256, ..., then the same fixed tree -- writes `out` and resets the arrival word.  The
// hand-off is the agent-scope one: partials are stored write-through (relaxed agent-scope atomic stores), drained, released; the last
// arriver acquires and reads them with agent-scope loads.  Partials are plain numbers: a NaN or Inf in a visible row reaches the mean.
//
// Face gradient: k_metric_bwd parks each splat's ONE contribution to its face (a double; +0.0 for an invisible splat) at the splat's CSR
// slot, coalesced reads and a scattered 8-byte write; k_metric_faces then gives 16 lanes to a face, lane l adds entries l, l + 16, ... of
// the face's contiguous run, and a fixed xor tree over the 16 lanes finishes the sum.  No float atomics anywhere.
//
// Compiled with -ffp-contract=off: the roundings per splat are the ones gms.h lists, whatever the compiler version, and the forward's u_j /
// v_j are bit for bit the values whose sign the backward's masks test (the backward recomputes them).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gms.h"
#include "launch_prof.h"
#include "lib_common.h"

namespace gms {

constexpr int BLOCK = 256;
constexpr int PER = 4;   // consecutive splats per lane
constexpr int SLAB = GMS_SLAB;
constexpr int WAVES = BLOCK / 64;
static_assert(SLAB == BLOCK * PER, "a slab is four splats per lane");
constexpr int SCRATCH_HEAD = 16;      // bytes: the arrival word, in a 16-byte block of its own at the start of the scratch
constexpr int PARTIAL_DOUBLES = 4;    // {sum m, sum b, count, unused} per workgroup
constexpr int FACE_LANES = 16;        // lanes that share one face in k_metric_faces
static_assert(GMS_ROW_BYTES == sizeof(double), "a parked contribution is one double");

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

// the lane's four entries of an index array (int32, or int64 when is64); entries past the end read as -1
template <bool VEC>
__device__ __forceinline__ void load_index(const void* __restrict__ b, int is64, long long i0, int nvalid, long long (&idx)[PER])
{
    if (VEC) {
        if (is64) {   // 32-byte steps from a 16-byte aligned base
            const longlong2* q = reinterpret_cast<const longlong2*>(static_cast<const long long*>(b) + i0);
            const longlong2 a = q[0], c = q[1];
            idx[0] = a.x, idx[1] = a.y, idx[2] = c.x, idx[3] = c.y;
        } else {      // 16-byte steps
            const int4 a = *reinterpret_cast<const int4*>(static_cast<const int*>(b) + i0);
            idx[0] = a.x, idx[1] = a.y, idx[2] = a.z, idx[3] = a.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k)
            idx[k] = k < nvalid ? (is64 ? static_cast<const long long*>(b)[i0 + k] : (long long)static_cast<const int*>(b)[i0 + k]) : -1;
    }
}

// f of the lane's four splats: face_scaling[binding] for a visible splat, NaN when its binding is outside [0, F) (never an out-of-bounds
// read), 0 for a splat that is invisible or past the end (never used)
__device__ __forceinline__ void gather_face(const float* __restrict__ fs, int F, const long long (&idx)[PER], unsigned m, float (&f)[PER])
{
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        f[k] = 0.f;
        if (m & (1u << k)) f[k] = (idx[k] >= 0 && idx[k] < (long long)F) ? fs[idx[k]] : __builtin_nanf("");
    }
}

template <typename T>
__device__ __forceinline__ T wave_sum(T x)   // fixed tree: lane 0 holds the sum of the wave's 64 values
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

__global__ __launch_bounds__(BLOCK) void k_metric_fwd(int P, int F, const float* __restrict__ xyz, const float* __restrict__ ls,
                                                      const float* __restrict__ fs, const void* __restrict__ binding, int is64,
                                                      const unsigned char* __restrict__ vis, float t_xyz, float t_s, int aligned, float* out,
                                                      unsigned* arrival, double* partials)
{
    __shared__ double sh[3 * WAVES + 1];   // (the one LDS object: wave partials, then the "I am last" word)
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = (int)blockIdx.x, nwg = (int)gridDim.x;
    const long long i0 = (long long)wg * SLAB + (long long)tid * PER;
    const long long left = (long long)P - i0;
    const int nvalid = left >= PER ? PER : (left > 0 ? (int)left : 0);
    const bool do_x = xyz != nullptr, do_s = ls != nullptr;                               // kernel arguments: scalar branches

    const bool vec = aligned && (long long)(wg + 1) * SLAB <= (long long)P;               // workgroup-uniform

    float X[3 * PER], S[3 * PER], f[PER];
    long long idx[PER];
    unsigned m;
    if (vec) {
        if (do_x) load_rows<true>(xyz, i0, nvalid, X);
        if (do_s) load_rows<true>(ls, i0, nvalid, S);
        load_index<true>(binding, is64, i0, nvalid, idx);
        m = load_visible<true>(vis, i0, nvalid);
    } else {
        if (do_x) load_rows<false>(xyz, i0, nvalid, X);
        if (do_s) load_rows<false>(ls, i0, nvalid, S);
        load_index<false>(binding, is64, i0, nvalid, idx);
        m = load_visible<false>(vis, i0, nvalid);
    }
    gather_face(fs, F, idx, m, f);

    double sa = 0.0, sb = 0.0, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (!(m & (1u << k))) continue;   // (an invisible row is never added, whatever it holds)
        cnt += 1.0;
        if (do_x) {
            const float u0 = relu(X[3 * k] * f[k] - t_xyz), u1 = relu(X[3 * k + 1] * f[k] - t_xyz), u2 = relu(X[3 * k + 2] * f[k] - t_xyz);
            sa += (double)sqrtf((u0 * u0 + u1 * u1) + u2 * u2);
        }
        if (do_s) {
            const float v0 = relu(expf(S[3 * k]) * f[k] - t_s), v1 = relu(expf(S[3 * k + 1]) * f[k] - t_s), v2 = relu(expf(S[3 * k + 2]) * f[k] - t_s);
            sb += (double)sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
        }
    }
    sa = wave_sum(sa), sb = wave_sum(sb), cnt = wave_sum(cnt);
    if (lane == 0) sh[3 * wave] = sa, sh[3 * wave + 1] = sb, sh[3 * wave + 2] = cnt;
    __syncthreads();
    if (tid == 0) {
        double pa = sh[0], pb = sh[1], pc = sh[2];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) pa += sh[3 * w], pb += sh[3 * w + 1], pc += sh[3 * w + 2];
        double* mine = partials + (long long)wg * PARTIAL_DOUBLES;
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

    // the last arriver: every partial, in a fixed order
    double da = 0.0, db = 0.0, dc = 0.0;
    for (int w = tid; w < nwg; w += BLOCK) {
        const double* q = partials + (long long)w * PARTIAL_DOUBLES;
        da += __hip_atomic_load(q + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        db += __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dc += __hip_atomic_load(q + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    da = wave_sum(da), db = wave_sum(db), dc = wave_sum(dc);
    __syncthreads();   // (sh[3 * WAVES] has been read by everybody; the wave slots are free again)
    if (lane == 0) sh[3 * wave] = da, sh[3 * wave + 1] = db, sh[3 * wave + 2] = dc;
    __syncthreads();
    if (tid == 0) {
        double ta = sh[0], tb = sh[1], tc = sh[2];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) ta += sh[3 * w], tb += sh[3 * w + 1], tc += sh[3 * w + 2];
        out[0] = do_x ? (float)(ta / tc) : 0.f;   // (tc == 0: 0 / 0 = NaN, the mean of an empty tensor)
        out[1] = do_s ? (float)(tb / tc) : 0.f;
        out[2] = (float)tc;
        out[3] = 0.f;
        __hip_atomic_store(arrival, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call, whatever the data held
    }
}

// live_x / live_s below: the term is on (its upstream gradient is given) and something is visible.  `rows` != nullptr: the face gradient
// is wanted, and EVERY splat inside the array parks its contribution (+0.0 when it has none) at rows[slot[i]].
__global__ __launch_bounds__(BLOCK) void k_metric_bwd(int P, int F, const float* __restrict__ xyz, const float* __restrict__ ls,
                                                      const float* __restrict__ fs, const void* __restrict__ binding, int is64,
                                                      const unsigned char* __restrict__ vis, float t_xyz, float t_s, int aligned,
                                                      const float* __restrict__ out, const float* __restrict__ g_xyz, const float* __restrict__ g_s,
                                                      float* __restrict__ d_xyz, float* __restrict__ d_ls, const int* __restrict__ slot,
                                                      double* __restrict__ rows)
{
    const int tid = (int)threadIdx.x;
    const long long i0 = (long long)blockIdx.x * SLAB + (long long)tid * PER;
    const long long left = (long long)P - i0;
    const int nvalid = left >= PER ? PER : (left > 0 ? (int)left : 0);
    if (nvalid == 0) return;

    const float c = out[2];
    const bool any = c > 0.f;                       // (c == 0: every gradient is +0, 1 / c is never formed)
    const bool live_x = g_xyz != nullptr && any, live_s = g_s != nullptr && any;
    const float kx = live_x ? g_xyz[0] / c : 0.f, ks = live_s ? g_s[0] / c : 0.f;

    const bool vec = aligned && (long long)(blockIdx.x + 1) * SLAB <= (long long)P;   // workgroup-uniform, as live_x / live_s

    float X[3 * PER], S[3 * PER], f[PER];
    long long idx[PER], sl[PER];
    unsigned m = 0u;
    if (vec) {
        if (live_x) load_rows<true>(xyz, i0, nvalid, X);
        if (live_s) load_rows<true>(ls, i0, nvalid, S);
        if (live_x || live_s) load_index<true>(binding, is64, i0, nvalid, idx), m = load_visible<true>(vis, i0, nvalid);
        if (rows) load_index<true>(slot, 0, i0, nvalid, sl);
    } else {
        if (live_x) load_rows<false>(xyz, i0, nvalid, X);
        if (live_s) load_rows<false>(ls, i0, nvalid, S);
        if (live_x || live_s) load_index<false>(binding, is64, i0, nvalid, idx), m = load_visible<false>(vis, i0, nvalid);
        if (rows) load_index<false>(slot, 0, i0, nvalid, sl);
    }
    if (live_x || live_s) gather_face(fs, F, idx, m, f);

    double W[PER] = {0.0, 0.0, 0.0, 0.0};   // the splat's contribution to d_face_scaling[binding]
    float DX[3 * PER], DS[3 * PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (live_x && (m & (1u << k))) {
            const float x0 = X[3 * k], x1 = X[3 * k + 1], x2 = X[3 * k + 2];
            const float u0 = relu(x0 * f[k] - t_xyz), u1 = relu(x1 * f[k] - t_xyz), u2 = relu(x2 * f[k] - t_xyz);
            const float mi = sqrtf((u0 * u0 + u1 * u1) + u2 * u2);
            if (mi > 0.f) {   // (the forward's fp32 norm decides; the quotients below use the norm of the same u in double)
                const double md = sqrt(((double)u0 * (double)u0 + (double)u1 * (double)u1) + (double)u2 * (double)u2);
                const double r0 = (double)u0 / md, r1 = (double)u1 / md, r2 = (double)u2 / md, kf = (double)kx * (double)f[k];
                if (u0 > 0.f) d0 = (float)(kf * r0);
                if (u1 > 0.f) d1 = (float)(kf * r1);
                if (u2 > 0.f) d2 = (float)(kf * r2);
                W[k] += (double)kx * ((r0 * (double)x0 + r1 * (double)x1) + r2 * (double)x2);
            }
        }
        DX[3 * k] = d0, DX[3 * k + 1] = d1, DX[3 * k + 2] = d2;
        d0 = d1 = d2 = 0.f;
        if (live_s && (m & (1u << k))) {
            const float e0 = expf(S[3 * k]), e1 = expf(S[3 * k + 1]), e2 = expf(S[3 * k + 2]);
            const float v0 = relu(e0 * f[k] - t_s), v1 = relu(e1 * f[k] - t_s), v2 = relu(e2 * f[k] - t_s);
            const float bi = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
            if (bi > 0.f) {
                const double bd = sqrt(((double)v0 * (double)v0 + (double)v1 * (double)v1) + (double)v2 * (double)v2);
                const double r0 = (double)v0 / bd, r1 = (double)v1 / bd, r2 = (double)v2 / bd, kf = (double)ks * (double)f[k];
                if (v0 > 0.f) d0 = (float)((kf * r0) * (double)e0);
                if (v1 > 0.f) d1 = (float)((kf * r1) * (double)e1);
                if (v2 > 0.f) d2 = (float)((kf * r2) * (double)e2);
                W[k] += (double)ks * ((r0 * (double)e0 + r1 * (double)e1) + r2 * (double)e2);
            }
        }
        DS[3 * k] = d0, DS[3 * k + 1] = d1, DS[3 * k + 2] = d2;
    }
    if (d_xyz) {
        if (vec) store_rows<true>(d_xyz, i0, nvalid, DX);
        else store_rows<false>(d_xyz, i0, nvalid, DX);
    }
    if (d_ls) {
        if (vec) store_rows<true>(d_ls, i0, nvalid, DS);
        else store_rows<false>(d_ls, i0, nvalid, DS);
    }
    if (rows) {
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (k < nvalid && sl[k] >= 0 && sl[k] < (long long)P) rows[sl[k]] = W[k];   // (a slot outside the array is never written)
    }
}

// d_face[f] = the sum of rows[face_begin[f] .. face_begin[f + 1]) in a fixed order, 16 lanes per face; +0.0 for a face without splats
__global__ __launch_bounds__(BLOCK) void k_metric_faces(int P, int F, const int* __restrict__ face_begin, const double* __restrict__ rows,
                                                        float* __restrict__ d_face)
{
    const long long gtid = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long f = gtid / FACE_LANES;
    const int sub = (int)(gtid % FACE_LANES);
    const bool okf = f < (long long)F;
    double acc = 0.0;
    if (okf) {
        int b0 = face_begin[f], b1 = face_begin[f + 1];
        b0 = b0 < 0 ? 0 : b0, b1 = b1 > P ? P : b1;   // (a run never leaves the array, whatever the table holds)
        for (int j = b0 + sub; j < b1; j += FACE_LANES) acc += rows[j];
    }
#pragma unroll
    for (int o = FACE_LANES / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, FACE_LANES);   // (every lane of the wave takes part)
    if (okf && sub == 0) d_face[f] = (float)acc;
}

}  // namespace gms

// ---------------------------------------------------------------------------------------------------------------
static inline bool aligned_to(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
static inline int64_t workgroups(int32_t P) { return P > 0 ? ((int64_t)P + gms::SLAB - 1) / gms::SLAB : 1; }

static int check_sizes(int32_t P, int32_t F)
{
    if (P < 0) return fail(GMS_E_ARG, "bad arguments: P < 0");
    if (P >= GMS_MAX_SPLATS) return fail(GMS_E_ARG, "bad arguments: P >= 2^24 (the count would not be an exact float)");
    if (F < 1) return fail(GMS_E_ARG, "bad arguments: F < 1");
    return GMS_OK;
}

extern "C" {

int gms_abi_version(void) { return GMS_ABI_VERSION; }
const char* gms_last_error(void) { return g_err; }

int64_t gms_scratch_bytes(int32_t P, int32_t F)
{
    if (check_sizes(P, F) != GMS_OK) return GMS_E_ARG;
    return (int64_t)gms::SCRATCH_HEAD + workgroups(P) * gms::PARTIAL_DOUBLES * (int64_t)sizeof(double);
}

int gms_forward(int32_t P, int32_t F, const void* xyz, const void* log_scaling, const void* face_scaling, const void* binding, int32_t index_is_i64,
                const void* visible, float threshold_xyz, float threshold_scale, void* out, void* scratch, void* stream_)
{
    if (check_sizes(P, F) != GMS_OK) return GMS_E_ARG;
    if (!out) return fail(GMS_E_ARG, "bad arguments: NULL out");
    if (!aligned_to(out, 4)) return fail(GMS_E_ARG, "bad arguments: out must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    if (P == 0) {   // no kernel: {NaN, NaN, 0, 0} by two fills on the stream
        hipError_t e = hipMemsetD32Async((hipDeviceptr_t)out, 0x7fc00000, 2, stream);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)((char*)out + 8), 0, 2, stream);
        if (e != hipSuccess) return fail(GMS_E_HIP, "gms_forward (P == 0): %s", hipGetErrorString(e));
        return GMS_OK;
    }
    if (!xyz && !log_scaling) return fail(GMS_E_ARG, "bad arguments: NULL xyz and NULL log_scaling (no term selected)");
    if (!face_scaling || !binding || !visible || !scratch) return fail(GMS_E_ARG, "bad arguments: NULL face_scaling, binding, visible or scratch");
    if (!aligned_to(xyz, 4) || !aligned_to(log_scaling, 4) || !aligned_to(face_scaling, 4) || !aligned_to(binding, index_is_i64 ? 8 : 4) ||
        !aligned_to(scratch, 16))
        return fail(GMS_E_ARG, "bad arguments: float pointers must be 4-byte aligned, binding aligned to its element, scratch 16-byte aligned");
    unsigned* arrival = (unsigned*)scratch;
    double* partials = (double*)((char*)scratch + gms::SCRATCH_HEAD);
    const dim3 grid((unsigned)workgroups(P)), block(gms::BLOCK);
    const int vec = aligned_to(xyz, 16) && aligned_to(log_scaling, 16) && aligned_to(binding, 16) && aligned_to(visible, 4);
    PROF_LAUNCH(gms::k_metric_fwd, grid, block, 0, stream, (int)P, (int)F, (const float*)xyz, (const float*)log_scaling, (const float*)face_scaling, binding,
                (int)(index_is_i64 != 0), (const unsigned char*)visible, threshold_xyz, threshold_scale, vec, (float*)out, arrival, partials);
    LAUNCH_CHECK(GMS_E_HIP, "k_metric_fwd");
    return GMS_OK;
}

int gms_backward(int32_t P, int32_t F, const void* xyz, const void* log_scaling, const void* face_scaling, const void* binding, int32_t index_is_i64,
                 const void* visible, float threshold_xyz, float threshold_scale, const void* out, const void* g_xyz, const void* g_scale, void* d_xyz,
                 void* d_log_scaling, void* d_face_scaling, const void* face_begin, const void* slot, void* rows, void* stream_)
{
    if (check_sizes(P, F) != GMS_OK) return GMS_E_ARG;
    if (!d_xyz && !d_log_scaling && !d_face_scaling) return GMS_OK;   // nothing to write
    hipStream_t stream = (hipStream_t)stream_;
    if (P == 0) {
        if (d_face_scaling) {
            if (!aligned_to(d_face_scaling, 4)) return fail(GMS_E_ARG, "bad arguments: every float pointer must be 4-byte aligned");
            const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)d_face_scaling, 0, (size_t)F, stream);
            if (e != hipSuccess) return fail(GMS_E_HIP, "gms_backward (P == 0): %s", hipGetErrorString(e));
        }
        return GMS_OK;
    }
    if (!out || !visible || !face_scaling || !binding) return fail(GMS_E_ARG, "bad arguments: NULL out, visible, face_scaling or binding");
    if (g_xyz && !xyz) return fail(GMS_E_ARG, "bad arguments: g_xyz given with NULL xyz");
    if (g_scale && !log_scaling) return fail(GMS_E_ARG, "bad arguments: g_scale given with NULL log_scaling");
    if (d_face_scaling && (!face_begin || !slot || !rows)) return fail(GMS_E_ARG, "bad arguments: d_face_scaling wanted with NULL face_begin, slot or rows");
    const void* four[] = {out, g_xyz, g_scale, g_xyz ? xyz : nullptr, g_scale ? log_scaling : nullptr, d_xyz, d_log_scaling, d_face_scaling, face_scaling,
                          face_begin, slot};
    for (const void* p : four)
        if (!aligned_to(p, 4)) return fail(GMS_E_ARG, "bad arguments: every float and int32 pointer must be 4-byte aligned");
    if (!aligned_to(binding, index_is_i64 ? 8 : 4) || !aligned_to(rows, 8))
        return fail(GMS_E_ARG, "bad arguments: binding must be aligned to its element, rows 8-byte aligned");
    // a term that is off is not read: its input does not decide the path
    const int vec = aligned_to(visible, 4) && aligned_to(binding, 16) && (!g_xyz || aligned_to(xyz, 16)) && (!g_scale || aligned_to(log_scaling, 16)) &&
                    aligned_to(d_xyz, 16) && aligned_to(d_log_scaling, 16) && (!d_face_scaling || aligned_to(slot, 16));
    const dim3 grid((unsigned)workgroups(P)), block(gms::BLOCK);
    PROF_LAUNCH(gms::k_metric_bwd, grid, block, 0, stream, (int)P, (int)F, (const float*)(g_xyz ? xyz : nullptr), (const float*)(g_scale ? log_scaling : nullptr),
                (const float*)face_scaling, binding, (int)(index_is_i64 != 0), (const unsigned char*)visible, threshold_xyz, threshold_scale, vec,
                (const float*)out, (const float*)g_xyz, (const float*)g_scale, (float*)d_xyz, (float*)d_log_scaling, (const int*)slot,
                (double*)(d_face_scaling ? rows : nullptr));
    LAUNCH_CHECK(GMS_E_HIP, "k_metric_bwd");
    if (d_face_scaling) {
        const int64_t threads = (int64_t)F * gms::FACE_LANES;
        PROF_LAUNCH(gms::k_metric_faces, dim3((unsigned)((threads + gms::BLOCK - 1) / gms::BLOCK)), block, 0, stream, (int)P, (int)F, (const int*)face_begin,
                    (const double*)rows, (float*)d_face_scaling);
        LAUNCH_CHECK(GMS_E_HIP, "k_metric_faces");
    }
    return GMS_OK;
}

LPROF_EXPORTS(gms)

}  // extern "C"

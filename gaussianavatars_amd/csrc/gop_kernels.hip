// gop_kernels.hip -- the fused Adam step of include/gop.h: one launch updates every tensor of every parameter group.
//
// Launch shape: one 256-thread workgroup per GOP_SLAB (2048) elements of one tensor.  The descriptor table rides in the kernel
// arguments; a workgroup finds its tensor by counting, over the whole (padded) prefix of work-unit counts, how many tensors end at or
// before its index -- 32 scalar compares on values the scalar unit loads in two instructions, no branch, the same answer in every lane.
// The slab is then streamed: every lane issues its eight 16-byte loads (two float4 of each of the four arrays) before the first use,
// 128 B per lane and 32 KiB per workgroup in flight; at the benchmark's 5.9 M elements that is 2 900 workgroups, eleven per CU.
// A slab's last partial float4 (the counts are 3N, 45N, N, ...: not multiples of four) is done element-wise by the first lanes, and
// so is a whole tensor whose four pointers are not all 16-byte aligned.  No LDS, no atomics.
//
// Compiled with -ffp-contract=off: the roundings per element are the ones gop.h lists -- its three fmaf() are written out, the compiler
// fuses nothing else -- whatever the compiler version.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/gop.h"
#include "launch_prof.h"
#include "lib_common.h"

namespace gop {

constexpr int T = GOP_MAX_TENSORS;
constexpr int BLOCK = 256;
constexpr int SLAB = GOP_SLAB;
constexpr int VEC_PER_LANE = SLAB / 4 / BLOCK;   // float4 per lane and array
constexpr int ELT_PER_LANE = SLAB / BLOCK;
static_assert(SLAB % (4 * BLOCK) == 0, "a slab is a whole number of float4 rounds");

struct Table {   // kernel argument, by value
    float* p[T];
    const float* g[T];
    float* m[T];
    float* v[T];
    long long n[T];
    float step_size[T];
    float bc2_sqrt[T];
    int unit_end[T];   // work units of tensors 0..i; INT_MAX past the last tensor
};
static_assert(sizeof(Table) + 5 * sizeof(float) <= 4096, "the table has to fit the kernel-argument segment");

struct Coef { float beta1, w1, beta2, w2, eps; };

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const Coef c, float neg_step, float bc2)
{
    m = fmaf(c.w1, g - m, m);
    v = v * c.beta2;
    v = fmaf(c.w2, g * g, v);
    const float q = sqrtf(v) / bc2 + c.eps;
    p = fmaf(neg_step, m / q, p);
}

__global__ __launch_bounds__(BLOCK) void k_adam(const Table t, const Coef c)
{
    const int wg = (int)blockIdx.x;
    int k = 0;
#pragma unroll
    for (int i = 0; i < T; ++i) k += wg >= t.unit_end[i] ? 1 : 0;   // wave-uniform; the padding keeps k < T
    const int first = k > 0 ? t.unit_end[k - 1] : 0;
    const long long base = (long long)(wg - first) * SLAB;
    const long long left = t.n[k] - base;
    const int count = left < SLAB ? (int)left : SLAB;   // >= 1 by construction of unit_end
    float* __restrict__ p = t.p[k] + base;
    const float* __restrict__ g = t.g[k] + base;
    float* __restrict__ m = t.m[k] + base;
    float* __restrict__ v = t.v[k] + base;
    const float neg_step = -t.step_size[k], bc2 = t.bc2_sqrt[k];
    const int tid = (int)threadIdx.x;

    // (base is a multiple of 2048 floats: a slab is aligned as its tensor is)
    const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
    if (aligned) {
        const int nvec = count >> 2;
        float4 P[VEC_PER_LANE], G[VEC_PER_LANE], M[VEC_PER_LANE], V[VEC_PER_LANE];
#pragma unroll
        for (int u = 0; u < VEC_PER_LANE; ++u) {
            const int j = tid + u * BLOCK;
            if (j < nvec) {
                G[u] = reinterpret_cast<const float4*>(g)[j];
                M[u] = reinterpret_cast<const float4*>(m)[j];
                V[u] = reinterpret_cast<const float4*>(v)[j];
                P[u] = reinterpret_cast<const float4*>(p)[j];
            }
        }
#pragma unroll
        for (int u = 0; u < VEC_PER_LANE; ++u) {
            const int j = tid + u * BLOCK;
            if (j < nvec) {
                adam1(P[u].x, G[u].x, M[u].x, V[u].x, c, neg_step, bc2);
                adam1(P[u].y, G[u].y, M[u].y, V[u].y, c, neg_step, bc2);
                adam1(P[u].z, G[u].z, M[u].z, V[u].z, c, neg_step, bc2);
                adam1(P[u].w, G[u].w, M[u].w, V[u].w, c, neg_step, bc2);
                reinterpret_cast<float4*>(m)[j] = M[u];
                reinterpret_cast<float4*>(v)[j] = V[u];
                reinterpret_cast<float4*>(p)[j] = P[u];
            }
        }
        const int i = (nvec << 2) + tid;   // the tail: at most three elements
        if (i < count) {
            float pe = p[i], me = m[i], ve = v[i];
            adam1(pe, g[i], me, ve, c, neg_step, bc2);
            m[i] = me, v[i] = ve, p[i] = pe;
        }
    } else {
        float P[ELT_PER_LANE], G[ELT_PER_LANE], M[ELT_PER_LANE], V[ELT_PER_LANE];
#pragma unroll
        for (int u = 0; u < ELT_PER_LANE; ++u) {
            const int i = tid + u * BLOCK;
            if (i < count) G[u] = g[i], M[u] = m[i], V[u] = v[i], P[u] = p[i];
        }
#pragma unroll
        for (int u = 0; u < ELT_PER_LANE; ++u) {
            const int i = tid + u * BLOCK;
            if (i < count) {
                adam1(P[u], G[u], M[u], V[u], c, neg_step, bc2);
                m[i] = M[u], v[i] = V[u], p[i] = P[u];
            }
        }
    }
}

}  // namespace gop

// ---------------------------------------------------------------------------------------------------------------
extern "C" {

int gop_abi_version(void) { return GOP_ABI_VERSION; }
const char* gop_last_error(void) { return g_err; }

int gop_adam_step_ex(int32_t ntensors, const GopAdamTensor* tensors, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                     float eps, void* stream_)
{
    if (ntensors < 0 || (ntensors > 0 && !tensors)) return fail(GOP_E_ARG, "bad arguments: ntensors < 0 or NULL table");
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f)) return fail(GOP_E_ARG, "bad arguments: betas outside [0, 1) or eps < 0");
    for (int32_t i = 0; i < ntensors; ++i) {
        const GopAdamTensor& a = tensors[i];
        if (a.n < 0) return fail(GOP_E_ARG, "tensor %d: n < 0", (int)i);
        if (a.n == 0) continue;
        if (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq) return fail(GOP_E_ARG, "tensor %d: NULL pointer", (int)i);
        if ((((uintptr_t)a.param) | ((uintptr_t)a.grad) | ((uintptr_t)a.exp_avg) | ((uintptr_t)a.exp_avg_sq)) & 3)
            return fail(GOP_E_ARG, "tensor %d: pointers must be 4-byte aligned", (int)i);
        if (!(a.bias_correction2_sqrt > 0.f)) return fail(GOP_E_ARG, "tensor %d: bias_correction2_sqrt must be > 0", (int)i);
    }
    const gop::Coef coef{beta1, one_minus_beta1, beta2, one_minus_beta2, eps};
    hipStream_t stream = (hipStream_t)stream_;
    int32_t i = 0;
    while (i < ntensors) {
        gop::Table t;
        int k = 0;
        long long units = 0;
        for (; i < ntensors && k < gop::T; ++i) {
            const GopAdamTensor& a = tensors[i];
            if (a.n == 0) continue;
            const long long u = (a.n + gop::SLAB - 1) / gop::SLAB;
            if (units + u >= (long long)INT_MAX) {
                if (k == 0) return fail(GOP_E_ARG, "tensor %d: too many elements for one launch", (int)i);
                break;   // the rest goes in the next launch
            }
            units += u;
            t.p[k] = (float*)a.param, t.g[k] = (const float*)a.grad, t.m[k] = (float*)a.exp_avg, t.v[k] = (float*)a.exp_avg_sq;
            t.n[k] = (long long)a.n, t.step_size[k] = a.step_size, t.bc2_sqrt[k] = a.bias_correction2_sqrt;
            t.unit_end[k] = (int)units;
            ++k;
        }
        if (k == 0) break;   // only empty tensors were left
        for (int j = k; j < gop::T; ++j) {
            t.p[j] = nullptr, t.g[j] = nullptr, t.m[j] = nullptr, t.v[j] = nullptr;
            t.n[j] = 0, t.step_size[j] = 0.f, t.bc2_sqrt[j] = 1.f, t.unit_end[j] = INT_MAX;
        }
        PROF_LAUNCH(gop::k_adam, dim3((unsigned)units), dim3(gop::BLOCK), 0, stream, t, coef);
        LAUNCH_CHECK(GOP_E_HIP, "k_adam");
    }
    return GOP_OK;
}

int gop_adam_step(int32_t ntensors, const GopAdamTensor* tensors, float beta1, float beta2, float eps, void* stream)
{
    return gop_adam_step_ex(ntensors, tensors, beta1, (float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2), eps, stream);
}

LPROF_EXPORTS(gop)

}  // extern "C"

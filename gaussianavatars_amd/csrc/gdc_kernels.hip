// gdc_kernels.hip -- adaptive density control of include/gdc.h: the reference's clone -> split -> prune sequence as
//
//   k_dc_decide    one thread per splat: the clone / split decision, the two prune-candidate flags (the row itself, its children) as a code
//                  byte, and the splat's contribution to its face's two counters (integer atomics: any order gives the same sums)
//   k_dc_resolve   the face protection: which candidates really go, hence the splat's four output counts (0 / 1 each: original, clone,
//                  child 0, child 1), the workgroup's four sums, and the new binding_counter
//   k_dc_scan_top  ONE workgroup turns the per-workgroup sums into exclusive offsets and posts the four totals (the block the host reads)
//   k_dc_apply     the scan's third step: every splat's output positions, written as the row map `src`
//   k_dc_gather    one launch for every tensor: 16 lanes share an output row and move it in 16-byte pieces (a row starts on a 4-byte
//                  boundary only -- 180 B rows -- so the pieces are typed 4-byte aligned and the compiler picks the widest legal access)
//   k_dc_permute   the gather's row mover on a plain permutation (gdc_permute): what the spatial re-sort moves a model's rows with
//
// The spatial order itself (gdc_morton_order: k_ord_*) is in gdc_order.h, the nearest-neighbour search on it (gdc_knn3_dist2: k_knn_*) in gdc_knn.h.
// No workgroup waits on another: the scan is three launches, not a look-back.  -ffp-contract=off: the decisions and the children's values
// round the way gdc.h lists, whatever the compiler would like to fuse.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gdc.h"
#include "launch_prof.h"
#include "lib_common.h"

namespace gdc {

constexpr int BLOCK = GDC_CHUNK;
constexpr int T = GDC_MAX_TENSORS;
constexpr int LANES = BLOCK / GDC_ROWS;   // lanes per output row
constexpr int WAVES = BLOCK / 64;
static_assert(BLOCK == 256 && LANES == 16, "the kernels are written for 256-thread workgroups of 64-lane waves");

// k_dc_decide's code byte
constexpr int C_CLONE = 1, C_SPLIT = 2, C_CAND = 4, C_CAND_CHILD = 8;
// k_dc_resolve's code byte: bit k = the splat emits a row into segment k
constexpr int SEGS = 4;

struct Thresholds { float max_grad, min_opacity, dense, big; int use_big; };   // dense = percent_dense * extent, big = 0.1 * extent

struct Table {   // kernel argument, by value
    const float* src[T];
    float* dst[T];
    int row_floats[T];
    int kind[T];
    int n;
};
static_assert(sizeof(Table) <= 1024, "the table has to fit the kernel-argument segment with room to spare");

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte piece on a 4-byte boundary

__device__ __forceinline__ int face_of(const void* binding, int is64, int i)
{
    return is64 ? (int)reinterpret_cast<const long long*>(binding)[i] : reinterpret_cast<const int*>(binding)[i];
}

__global__ __launch_bounds__(BLOCK) void k_dc_decide(int P, int F, const Thresholds th, const float* __restrict__ scaling,
                                                     const float* __restrict__ opacity, const float* __restrict__ accum,
                                                     const float* __restrict__ denom, const void* __restrict__ binding, int is64,
                                                     const float* __restrict__ face_scaling, int* __restrict__ cnt, int* __restrict__ cand,
                                                     unsigned char* __restrict__ code)
{
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= P) return;
    int f = -1;
    float fs = 1.f;
    if (binding) {
        f = face_of(binding, is64, i);
        if ((unsigned)f >= (unsigned)F) {   // a binding outside the mesh: the row is kept as it is and touches no counter
            code[i] = 0;
            return;
        }
        fs = face_scaling[f];
    }
    float g = accum[i] / denom[i];
    if (g != g) g = 0.f;
    float w[3], S = 0.f, Sc = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float e = expf(scaling[3 * i + j]);
        w[j] = binding ? e * fs : e;
        S = j == 0 ? w[j] : fmaxf(S, w[j]);
        const float c = logf((binding ? w[j] / fs : e) / 1.6f);   // the child's stored log-scale, and the world scale it reads back as
        const float wc = binding ? expf(c) * fs : expf(c);
        Sc = j == 0 ? wc : fmaxf(Sc, wc);
    }
    const float o = 1.f / (1.f + expf(-opacity[i]));
    const bool clone = fabsf(g) >= th.max_grad && S <= th.dense;
    const bool split = g >= th.max_grad && S > th.dense;
    const bool low = o < th.min_opacity;
    const bool c_row = low || (th.use_big && S > th.big);
    const bool c_child = low || (th.use_big && Sc > th.big);
    code[i] = (unsigned char)((clone ? C_CLONE : 0) | (split ? C_SPLIT : 0) | (c_row ? C_CAND : 0) | (c_child ? C_CAND_CHILD : 0));
    if (binding) {
        if (clone || split) atomicAdd(&cnt[f], 1);   // a copy more; two children for one original
        const int dc = split ? (c_child ? 2 : 0) : (c_row ? (clone ? 2 : 1) : 0);
        if (dc) atomicAdd(&cand[f], dc);
    }
}

__global__ __launch_bounds__(BLOCK) void k_dc_resolve(int P, int F, int nchunks, const void* __restrict__ binding, int is64,
                                                      const int* __restrict__ cnt, const int* __restrict__ cand, unsigned char* __restrict__ code,
                                                      int* __restrict__ sums, int* __restrict__ counter_out)
{
    __shared__ int part[WAVES][SEGS];
    const int tid = (int)threadIdx.x;
    const int i = (int)(blockIdx.x * BLOCK) + tid;
    if (i < F) {
        const int n = cnt[i], c = cand[i];
        counter_out[i] = n - c > 0 ? n - c : n;
    }
    int bits = 0;
    if (i < P) {
        const int c = code[i];
        bool remove = true;
        if (binding) {
            const int f = face_of(binding, is64, i);
            remove = (unsigned)f < (unsigned)F && cnt[f] - cand[f] > 0;
        }
        if (c & C_SPLIT) {
            bits = ((c & C_CAND_CHILD) && remove) ? 0 : (4 | 8);
        } else {
            const bool keep = !((c & C_CAND) && remove);
            bits = keep ? (1 | ((c & C_CLONE) ? 2 : 0)) : 0;
        }
        code[i] = (unsigned char)bits;
    }
    if ((int)blockIdx.x >= nchunks) return;   // (workgroup-uniform: the extra workgroups only serve the faces)
#pragma unroll
    for (int k = 0; k < SEGS; ++k) {
        const int n = __popcll(__ballot((bits >> k) & 1));
        if ((tid & 63) == 0) part[tid >> 6][k] = n;
    }
    __syncthreads();
    if (tid < SEGS) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += part[w][tid];
        sums[(int)blockIdx.x * SEGS + tid] = s;
    }
}

// one workgroup: sums[chunk][k] -> the exclusive prefix over the chunks, totals[k] = the sum over all of them
__global__ __launch_bounds__(BLOCK) void k_dc_scan_top(int nchunks, int* __restrict__ sums, int* __restrict__ totals)
{
    __shared__ int lane_sum[BLOCK][SEGS];
    const int tid = (int)threadIdx.x;
    const int per = (nchunks + BLOCK - 1) / BLOCK;
    const int lo = tid * per < nchunks ? tid * per : nchunks;
    const int hi = lo + per < nchunks ? lo + per : nchunks;
    int mine[SEGS] = {0, 0, 0, 0};
    for (int c = lo; c < hi; ++c)
#pragma unroll
        for (int k = 0; k < SEGS; ++k) mine[k] += sums[c * SEGS + k];
#pragma unroll
    for (int k = 0; k < SEGS; ++k) lane_sum[tid][k] = mine[k];
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {   // inclusive scan over the 256 threads
        int add[SEGS] = {0, 0, 0, 0};
        if (tid >= d)
#pragma unroll
            for (int k = 0; k < SEGS; ++k) add[k] = lane_sum[tid - d][k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SEGS; ++k) lane_sum[tid][k] += add[k];
        __syncthreads();
    }
    int run[SEGS];
#pragma unroll
    for (int k = 0; k < SEGS; ++k) run[k] = lane_sum[tid][k] - mine[k];
    for (int c = lo; c < hi; ++c)
#pragma unroll
        for (int k = 0; k < SEGS; ++k) {
            const int v = sums[c * SEGS + k];
            sums[c * SEGS + k] = run[k];
            run[k] += v;
        }
    if (tid < SEGS) totals[tid] = lane_sum[BLOCK - 1][tid];
}

struct Seg { int base[SEGS]; int N; };

__global__ __launch_bounds__(BLOCK) void k_dc_apply(int P, const Seg seg, const unsigned char* __restrict__ code, const int* __restrict__ sums,
                                                    int* __restrict__ src)
{
    __shared__ int part[WAVES][SEGS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = (int)(blockIdx.x * BLOCK) + tid;
    const int bits = i < P ? code[i] : 0;
    int before[SEGS];
#pragma unroll
    for (int k = 0; k < SEGS; ++k) {
        const unsigned long long m = __ballot((bits >> k) & 1);
        before[k] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) part[wave][k] = __popcll(m);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SEGS; ++k) {
        if (!((bits >> k) & 1)) continue;
        int pos = seg.base[k] + sums[(int)blockIdx.x * SEGS + k] + before[k];
        for (int w = 0; w < wave; ++w) pos += part[w][k];
        if (pos < seg.N) src[pos] = k == 0 ? i : -1 - i;
    }
}

// lane `sub` of the 16 that share a row: rf 4-byte elements from a (or +0.0) to d, in 16-byte pieces and a tail of single elements
__device__ __forceinline__ void move_row(float* __restrict__ d, const float* __restrict__ a, int rf, int sub, bool zero)
{
    const int np = rf >> 2;
    for (int p = sub; p < np; p += LANES) {
        f4u v = {0.f, 0.f, 0.f, 0.f};
        if (!zero) v = *reinterpret_cast<const f4u*>(a + 4 * p);
        *reinterpret_cast<f4u*>(d + 4 * p) = v;
    }
    const int e = (np << 2) + sub;
    if (e < rf) d[e] = zero ? 0.f : a[e];
}

__global__ __launch_bounds__(BLOCK) void k_dc_gather(const Table t, int P, const Seg seg, const int* __restrict__ srcmap,
                                                     const float* __restrict__ xyz, const float* __restrict__ scaling,
                                                     const float* __restrict__ rotation, const float* __restrict__ noise,
                                                     const void* __restrict__ binding, int is64, const float* __restrict__ face_scaling,
                                                     float* __restrict__ xyz_out, float* __restrict__ scaling_out, void* __restrict__ binding_out)
{
    const int tid = (int)threadIdx.x, sub = tid & (LANES - 1);
    const int row = (int)(blockIdx.x * GDC_ROWS) + (tid >> 4);
    if (row >= seg.N) return;
    const int s = srcmap[row];
    const bool born = s < 0;
    const int source = born ? -1 - s : s;
    if ((unsigned)source >= (unsigned)P) return;
    const bool child = row >= seg.base[2];
    for (int k = 0; k < t.n; ++k) {
        const int rf = t.row_floats[k], kind = t.kind[k];
        if (child && (kind == GDC_XYZ || kind == GDC_SCALING)) continue;   // written below
        const bool zero = kind == GDC_ZERO || (kind == GDC_MOMENT && born);
        move_row(t.dst[k] + (size_t)row * rf, zero ? nullptr : t.src[k] + (size_t)source * rf, rf, sub, zero);
    }
    if (binding && sub == 1) {
        if (is64) reinterpret_cast<long long*>(binding_out)[row] = reinterpret_cast<const long long*>(binding)[source];
        else reinterpret_cast<int*>(binding_out)[row] = reinterpret_cast<const int*>(binding)[source];
    }
    if (child && sub == 0) {
        const int c = row >= seg.base[3] ? 1 : 0;
        const float fs = binding ? face_scaling[face_of(binding, is64, source)] : 1.f;   // (k_dc_decide splits no row whose face is outside the mesh)
        float w[3], smp[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float e = expf(scaling[3 * (size_t)source + j]);
            w[j] = binding ? e * fs : e;
            smp[j] = noise[((size_t)c * P + source) * 3 + j] * w[j];
            scaling_out[3 * (size_t)row + j] = logf((binding ? w[j] / fs : e) / 1.6f);
        }
        float r = rotation[4 * (size_t)source], x = rotation[4 * (size_t)source + 1], y = rotation[4 * (size_t)source + 2],
              z = rotation[4 * (size_t)source + 3];
        const float nrm = sqrtf(r * r + x * x + y * y + z * z);
        r /= nrm, x /= nrm, y /= nrm, z /= nrm;
        const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                               {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                               {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
#pragma unroll
        for (int j = 0; j < 3; ++j)
            xyz_out[3 * (size_t)row + j] = (R[j][0] * smp[0] + R[j][1] * smp[1] + R[j][2] * smp[2]) + xyz[3 * (size_t)source + j];
    }
}

// gdc_permute: dst[r] = src[perm[r]] for every tensor of the table, on the gather's row mover; an index outside [0, P) reads nothing: +0.0
__global__ __launch_bounds__(BLOCK) void k_dc_permute(const Table t, int P, const int* __restrict__ perm)
{
    const int tid = (int)threadIdx.x, sub = tid & (LANES - 1);
    const int row = (int)(blockIdx.x * GDC_ROWS) + (tid >> 4);
    if (row >= P) return;
    const int source = perm[row];
    const bool zero = (unsigned)source >= (unsigned)P;
    for (int k = 0; k < t.n; ++k) {
        const int rf = t.row_floats[k];
        move_row(t.dst[k] + (size_t)row * rf, zero ? nullptr : t.src[k] + (size_t)source * rf, rf, sub, zero);
    }
}

// the workspace, in 4-byte units: totals[4] | cnt[F] | cand[F] | sums[4 * nchunks] | code[P bytes]
struct Workspace { int* totals; int* cnt; int* cand; int* sums; unsigned char* code; int nchunks; };

static Workspace carve(void* base, int P, int F)
{
    Workspace w;
    w.nchunks = (P + BLOCK - 1) / BLOCK;
    w.totals = (int*)base;
    w.cnt = w.totals + 4;
    w.cand = w.cnt + F;
    w.sums = w.cand + F;
    w.code = (unsigned char*)(w.sums + (size_t)SEGS * w.nchunks);
    return w;
}

}  // namespace gdc

#include "gdc_order.h"
#include "gdc_knn.h"

#define HIP_CHECK(call, what)                                                                 \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) return fail(GDC_E_HIP, "%s: %s", what, hipGetErrorString(e_));  \
    } while (0)

// the fifteen launches of the spatial order (gdc_morton_order, and the first step of gdc_knn3_dist2): arguments already checked
static int enqueue_order(int P, int F, const void* xyz, const void* binding, int is64, const void* face_centers, void* perm_out, void* workspace,
                         hipStream_t stream)
{
    const gdc::OrderWorkspace w = gdc::carve_order(workspace, P);
    const dim3 grid((unsigned)w.nchunks), block(gdc::BLOCK);
    PROF_LAUNCH(gdc::k_ord_clear, dim3((gdc::ORD_HEAD + gdc::BLOCK - 1) / gdc::BLOCK), block, 0, stream, (int*)w.box);
    LAUNCH_CHECK(GDC_E_HIP, "k_ord_clear");
    PROF_LAUNCH(gdc::k_ord_bounds, grid, block, 0, stream, (int)P, (int)F, (const float*)xyz, binding, is64,
                (const float*)face_centers, w.box);
    LAUNCH_CHECK(GDC_E_HIP, "k_ord_bounds");
    PROF_LAUNCH(gdc::k_ord_codes, grid, block, 0, stream, (int)P, (int)F, (const float*)xyz, binding, is64,
                (const float*)face_centers, (const unsigned*)w.box, w.keys[0]);
    LAUNCH_CHECK(GDC_E_HIP, "k_ord_codes");
    for (int pass = 0; pass < gdc::PASSES; ++pass) {   // keys ping-pong between the two buffers; the last pass writes the rows to perm_out
        const int shift = pass * gdc::RADIX_BITS, in = pass & 1, out = in ^ 1;
        const bool last = pass == gdc::PASSES - 1;
        int* totals = w.totals + pass * gdc::RADIX;
        PROF_LAUNCH(gdc::k_ord_hist, grid, block, 0, stream, (int)P, w.nchunks, shift, (const unsigned*)w.keys[in], w.table, totals);
        LAUNCH_CHECK(GDC_E_HIP, "k_ord_hist");
        PROF_LAUNCH(gdc::k_ord_scan, dim3(gdc::RADIX), block, 0, stream, w.nchunks, w.table, (const int*)totals);
        LAUNCH_CHECK(GDC_E_HIP, "k_ord_scan");
        PROF_LAUNCH(gdc::k_ord_scatter, grid, block, 0, stream, (int)P, w.nchunks, shift, (const unsigned*)w.keys[in],
                    (const int*)(pass == 0 ? nullptr : w.vals[in]), (const int*)w.table, last ? (unsigned*)nullptr : w.keys[out],
                    last ? (int*)perm_out : w.vals[out]);
        LAUNCH_CHECK(GDC_E_HIP, "k_ord_scatter");
    }
    return GDC_OK;
}

// ---------------------------------------------------------------------------------------------------------------
extern "C" {

int gdc_abi_version(void) { return GDC_ABI_VERSION; }
const char* gdc_last_error(void) { return g_err; }

int64_t gdc_workspace_bytes(int32_t P, int32_t F)
{
    if (P < 0 || F < 0 || P >= GDC_MAX_SPLATS) return -1;
    const int64_t nchunks = ((int64_t)P + gdc::BLOCK - 1) / gdc::BLOCK;
    return 4 * (4 + 2 * (int64_t)F + gdc::SEGS * nchunks) + (((int64_t)P + 3) & ~(int64_t)3);
}

static bool misaligned(const void* p) { return (((uintptr_t)p) & 3) != 0; }

int gdc_plan(int32_t P, int32_t F, const GdcParams* params, const void* scaling, const void* opacity, const void* accum, const void* denom,
             const void* binding, int32_t binding_is_i64, const void* face_scaling, const void* binding_counter, void* counter_out,
             void* workspace, int32_t* totals, void* stream_)
{
    if (!totals) return fail(GDC_E_ARG, "bad arguments: NULL totals");
    totals[0] = totals[1] = totals[2] = totals[3] = 0;
    if (P < 0 || P >= GDC_MAX_SPLATS || F < 0) return fail(GDC_E_ARG, "bad arguments: P = %d outside [0, %d) or F = %d < 0", (int)P, GDC_MAX_SPLATS, (int)F);
    if (!params) return fail(GDC_E_ARG, "bad arguments: NULL params");
    if (!(params->max_grad > 0.f)) return fail(GDC_E_ARG, "bad arguments: max_grad must be > 0 (a clone's zero gradient must not select it again)");
    if (!(params->extent >= 0.f) || !(params->percent_dense >= 0.f) || !(params->max_screen_size >= 0.f) || params->min_opacity != params->min_opacity)
        return fail(GDC_E_ARG, "bad arguments: extent, percent_dense and max_screen_size must be >= 0 and min_opacity a number");
    if (binding && (F <= 0 || !face_scaling || !binding_counter || !counter_out))
        return fail(GDC_E_ARG, "bad arguments: a bound model needs F > 0, face_scaling, binding_counter and counter_out");
    if (P == 0) {   // nothing is launched; the counters of a bound model carry over (an empty binding may well be a NULL pointer: F decides)
        if (F > 0 && binding_counter && counter_out && counter_out != binding_counter)
            HIP_CHECK(hipMemcpyAsync(counter_out, binding_counter, sizeof(int) * (size_t)F, hipMemcpyDeviceToDevice, (hipStream_t)stream_), "counter copy");
        return GDC_OK;
    }
    if (!binding) F = 0;
    if (!scaling || !opacity || !accum || !denom || !workspace) return fail(GDC_E_ARG, "bad arguments: NULL pointer");
    if (misaligned(scaling) || misaligned(opacity) || misaligned(accum) || misaligned(denom) || misaligned(workspace) || misaligned(face_scaling) ||
        misaligned(binding_counter) || misaligned(counter_out) || (((uintptr_t)binding) & (binding_is_i64 ? 7 : 3)))
        return fail(GDC_E_ARG, "bad arguments: pointers must be aligned to their element");
    hipStream_t stream = (hipStream_t)stream_;
    const gdc::Workspace w = gdc::carve(workspace, P, F);
    const gdc::Thresholds th{params->max_grad, params->min_opacity, (float)((double)params->percent_dense * (double)params->extent),
                             (float)(0.1 * (double)params->extent), params->max_screen_size != 0.f ? 1 : 0};
    if (F > 0) {
        HIP_CHECK(hipMemcpyAsync(w.cnt, binding_counter, sizeof(int) * (size_t)F, hipMemcpyDeviceToDevice, stream), "counter copy");
        HIP_CHECK(hipMemsetAsync(w.cand, 0, sizeof(int) * (size_t)F, stream), "counter clear");
    }
    const int fblocks = (F + gdc::BLOCK - 1) / gdc::BLOCK;
    PROF_LAUNCH(gdc::k_dc_decide, dim3((unsigned)w.nchunks), dim3(gdc::BLOCK), 0, stream, (int)P, (int)F, th, (const float*)scaling,
                (const float*)opacity, (const float*)accum, (const float*)denom, binding, (int)binding_is_i64, (const float*)face_scaling, w.cnt,
                w.cand, w.code);
    LAUNCH_CHECK(GDC_E_HIP, "k_dc_decide");
    PROF_LAUNCH(gdc::k_dc_resolve, dim3((unsigned)(w.nchunks > fblocks ? w.nchunks : fblocks)), dim3(gdc::BLOCK), 0, stream, (int)P, (int)F,
                w.nchunks, binding, (int)binding_is_i64, (const int*)w.cnt, (const int*)w.cand, w.code, w.sums, (int*)counter_out);
    LAUNCH_CHECK(GDC_E_HIP, "k_dc_resolve");
    PROF_LAUNCH(gdc::k_dc_scan_top, dim3(1), dim3(gdc::BLOCK), 0, stream, w.nchunks, w.sums, w.totals);
    LAUNCH_CHECK(GDC_E_HIP, "k_dc_scan_top");
    HIP_CHECK(hipMemcpyAsync(totals, w.totals, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, stream), "totals read");
    HIP_CHECK(hipStreamSynchronize(stream), "totals read");
    return GDC_OK;
}

int gdc_emit(int32_t P, int32_t F, const int32_t* totals, int32_t ntensors, const GdcTensor* tensors, const void* xyz, const void* scaling,
             const void* rotation, const void* noise, const void* binding, int32_t binding_is_i64, const void* face_scaling, void* src_out,
             void* binding_out, void* workspace, void* stream_)
{
    if (P < 0 || P >= GDC_MAX_SPLATS || F < 0 || !totals) return fail(GDC_E_ARG, "bad arguments: P outside [0, %d), F < 0 or NULL totals", GDC_MAX_SPLATS);
    if (ntensors < 0 || ntensors > GDC_MAX_TENSORS || (ntensors > 0 && !tensors))
        return fail(GDC_E_ARG, "bad arguments: ntensors outside [0, %d] or NULL table", GDC_MAX_TENSORS);
    gdc::Seg seg;
    int64_t N = 0;
    for (int k = 0; k < gdc::SEGS; ++k) {
        if (totals[k] < 0 || totals[k] > P) return fail(GDC_E_ARG, "bad arguments: totals[%d] = %d outside [0, P]", k, (int)totals[k]);
        seg.base[k] = (int)N;
        N += totals[k];
    }
    if (totals[2] != totals[3] || (int64_t)totals[0] + totals[2] > P || (int64_t)totals[1] + totals[2] > P)
        return fail(GDC_E_ARG, "bad arguments: totals that no plan reports");
    seg.N = (int)N;
    if (N == 0) return GDC_OK;
    if (!src_out || !workspace || !xyz || !scaling || !rotation || !noise) return fail(GDC_E_ARG, "bad arguments: NULL pointer");
    if (binding && (!face_scaling || !binding_out)) return fail(GDC_E_ARG, "bad arguments: a bound model needs face_scaling and binding_out");
    if (misaligned(src_out) || misaligned(workspace) || misaligned(xyz) || misaligned(scaling) || misaligned(rotation) || misaligned(noise) ||
        misaligned(face_scaling) || (((uintptr_t)binding | (uintptr_t)binding_out) & (binding_is_i64 ? 7 : 3)))
        return fail(GDC_E_ARG, "bad arguments: pointers must be aligned to their element");
    gdc::Table t;
    float *xyz_out = nullptr, *scaling_out = nullptr;
    for (int k = 0; k < gdc::T; ++k) {
        t.src[k] = nullptr, t.dst[k] = nullptr, t.row_floats[k] = 0, t.kind[k] = GDC_ZERO;
        if (k >= ntensors) continue;
        const GdcTensor& a = tensors[k];
        if (a.row_floats < 0 || a.kind < GDC_COPY || a.kind > GDC_SCALING) return fail(GDC_E_ARG, "tensor %d: bad row_floats or kind", k);
        if (a.row_floats > 0 && (!a.dst || (a.kind != GDC_ZERO && !a.src))) return fail(GDC_E_ARG, "tensor %d: NULL pointer", k);
        if (misaligned(a.src) || misaligned(a.dst)) return fail(GDC_E_ARG, "tensor %d: pointers must be 4-byte aligned", k);
        if (a.kind == GDC_XYZ || a.kind == GDC_SCALING) {
            float*& slot = a.kind == GDC_XYZ ? xyz_out : scaling_out;
            if (slot || a.row_floats != 3) return fail(GDC_E_ARG, "tensor %d: one GDC_XYZ and one GDC_SCALING tensor, three floats per row", k);
            slot = (float*)a.dst;
        }
        t.src[k] = (const float*)a.src, t.dst[k] = (float*)a.dst, t.row_floats[k] = a.row_floats, t.kind[k] = a.kind;
    }
    t.n = ntensors;
    if (totals[2] > 0 && (!xyz_out || !scaling_out)) return fail(GDC_E_ARG, "bad arguments: children need the GDC_XYZ and the GDC_SCALING tensor");
    hipStream_t stream = (hipStream_t)stream_;
    const gdc::Workspace w = gdc::carve(workspace, P, binding ? F : 0);
    PROF_LAUNCH(gdc::k_dc_apply, dim3((unsigned)w.nchunks), dim3(gdc::BLOCK), 0, stream, (int)P, seg, (const unsigned char*)w.code,
                (const int*)w.sums, (int*)src_out);
    LAUNCH_CHECK(GDC_E_HIP, "k_dc_apply");
    PROF_LAUNCH(gdc::k_dc_gather, dim3((unsigned)((N + GDC_ROWS - 1) / GDC_ROWS)), dim3(gdc::BLOCK), 0, stream, t, (int)P, seg,
                (const int*)src_out, (const float*)xyz, (const float*)scaling, (const float*)rotation, (const float*)noise, binding,
                (int)binding_is_i64, (const float*)face_scaling, xyz_out, scaling_out, binding_out);
    LAUNCH_CHECK(GDC_E_HIP, "k_dc_gather");
    return GDC_OK;
}

int64_t gdc_order_workspace_bytes(int32_t P)
{
    if (P < 0 || P >= GDC_MAX_SPLATS) return -1;
    const int64_t nchunks = ((int64_t)P + gdc::BLOCK - 1) / gdc::BLOCK;
    return 4 * (gdc::ORD_HEAD + 4 * (int64_t)P + gdc::RADIX * nchunks);
}

int gdc_morton_order(int32_t P, int32_t F, const void* xyz, const void* binding, int32_t binding_is_i64, const void* face_centers,
                     void* perm_out, void* workspace, void* stream_)
{
    if (P < 0 || P >= GDC_MAX_SPLATS || F < 0) return fail(GDC_E_ARG, "bad arguments: P = %d outside [0, %d) or F = %d < 0", (int)P, GDC_MAX_SPLATS, (int)F);
    if ((binding != nullptr) != (face_centers != nullptr) || (binding && F <= 0))
        return fail(GDC_E_ARG, "bad arguments: a bound model needs binding, face_centers and F > 0; an unbound one neither pointer");
    if (P == 0) return GDC_OK;
    if (!xyz || !perm_out || !workspace) return fail(GDC_E_ARG, "bad arguments: NULL pointer");
    if (misaligned(xyz) || misaligned(perm_out) || misaligned(workspace) || misaligned(face_centers) || (((uintptr_t)binding) & (binding_is_i64 ? 7 : 3)))
        return fail(GDC_E_ARG, "bad arguments: pointers must be aligned to their element");
    return enqueue_order(P, F, xyz, binding, binding_is_i64, face_centers, perm_out, workspace, (hipStream_t)stream_);
}

int gdc_permute(int32_t P, const void* perm, int32_t ntensors, const GdcTensor* tensors, void* stream_)
{
    if (P < 0 || P >= GDC_MAX_SPLATS) return fail(GDC_E_ARG, "bad arguments: P = %d outside [0, %d)", (int)P, GDC_MAX_SPLATS);
    if (ntensors < 0 || ntensors > GDC_MAX_TENSORS || (ntensors > 0 && !tensors))
        return fail(GDC_E_ARG, "bad arguments: ntensors outside [0, %d] or NULL table", GDC_MAX_TENSORS);
    if (P == 0 || ntensors == 0) return GDC_OK;
    if (!perm) return fail(GDC_E_ARG, "bad arguments: NULL pointer");
    if (misaligned(perm)) return fail(GDC_E_ARG, "bad arguments: pointers must be aligned to their element");
    gdc::Table t;
    for (int k = 0; k < gdc::T; ++k) {
        t.src[k] = nullptr, t.dst[k] = nullptr, t.row_floats[k] = 0, t.kind[k] = GDC_COPY;
        if (k >= ntensors) continue;
        const GdcTensor& a = tensors[k];
        if (a.row_floats < 0 || a.kind != GDC_COPY) return fail(GDC_E_ARG, "tensor %d: bad row_floats, or a kind other than GDC_COPY", k);
        if (a.row_floats > 0 && (!a.dst || !a.src)) return fail(GDC_E_ARG, "tensor %d: NULL pointer", k);
        if (misaligned(a.src) || misaligned(a.dst)) return fail(GDC_E_ARG, "tensor %d: pointers must be 4-byte aligned", k);
        t.src[k] = (const float*)a.src, t.dst[k] = (float*)a.dst, t.row_floats[k] = a.row_floats;
    }
    t.n = ntensors;
    PROF_LAUNCH(gdc::k_dc_permute, dim3((unsigned)(((int64_t)P + GDC_ROWS - 1) / GDC_ROWS)), dim3(gdc::BLOCK), 0, (hipStream_t)stream_, t, (int)P,
                (const int*)perm);
    LAUNCH_CHECK(GDC_E_HIP, "k_dc_permute");
    return GDC_OK;
}

int64_t gdc_knn_workspace_bytes(int32_t P)
{
    if (P < 0 || P >= GDC_MAX_SPLATS) return -1;
    const int64_t nboxes = ((int64_t)P + gdc::KNN_CHUNK - 1) / gdc::KNN_CHUNK;
    return 16 * (int64_t)P + 32 * nboxes + 4 * (int64_t)P + gdc_order_workspace_bytes(P);
}

int gdc_knn3_dist2(int32_t P, const void* xyz, void* dist2_out, void* workspace, void* stream_)
{
    if (P < 0 || P >= GDC_MAX_SPLATS) return fail(GDC_E_ARG, "bad arguments: P = %d outside [0, %d)", (int)P, GDC_MAX_SPLATS);
    if (P == 0) return GDC_OK;
    if (!xyz || !dist2_out || !workspace) return fail(GDC_E_ARG, "bad arguments: NULL pointer");
    if (misaligned(xyz) || misaligned(dist2_out) || (((uintptr_t)workspace) & 15))
        return fail(GDC_E_ARG, "bad arguments: pointers must be aligned to their element, the workspace to 16 bytes");
    hipStream_t stream = (hipStream_t)stream_;
    const gdc::KnnWorkspace w = gdc::carve_knn(workspace, P);
    const int rc = enqueue_order(P, 0, xyz, nullptr, 0, nullptr, w.perm, w.order, stream);
    if (rc != GDC_OK) return rc;
    const dim3 grid((unsigned)(((int64_t)P + gdc::BLOCK - 1) / gdc::BLOCK)), block(gdc::BLOCK);
    PROF_LAUNCH(gdc::k_knn_gather, grid, block, 0, stream, (int)P, (const float*)xyz, (const int*)w.perm, w.pts, w.boxes);
    LAUNCH_CHECK(GDC_E_HIP, "k_knn_gather");
    PROF_LAUNCH(gdc::k_knn_search, grid, block, 0, stream, (int)P, w.nboxes, (const gdc::f4a*)w.pts, (const gdc::f4a*)w.boxes, (const int*)w.perm,
                (float*)dist2_out);
    LAUNCH_CHECK(GDC_E_HIP, "k_knn_search");
    return GDC_OK;
}

LPROF_EXPORTS(gdc)

}  // extern "C"

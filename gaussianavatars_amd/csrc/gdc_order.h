// gdc_order.h -- the spatial order of include/gdc.h (gdc_morton_order): io.morton_order's permutation, bit for bit, without leaving the device.
//
//   k_ord_clear     the head of the workspace (the box and the digit totals of the four passes) to zero: kernels only, so that a recorded
//                   call has no memset node
//   k_ord_bounds    one thread per splat: its fp32 position, the workgroup's per-axis min / max, six integer atomics per workgroup on an
//                   order-preserving encoding of the floats (min and max are exact: any order of the atomics gives the same bits)
//   k_ord_codes     the position again (same two roundings), quantised in fp64 the way numpy does it, interleaved to the 30-bit code
//   k_ord_hist      one LSD pass, step 1: the workgroup's count per 8-bit digit into table[digit][workgroup], and the digit's total
//   k_ord_scan      step 2, one workgroup per digit: its row of the table -> exclusive offsets, behind the totals of every smaller digit
//   k_ord_scatter   step 3: key and row to offset + rank, the rank by a ballot match per digit bit -- lanes of a wave in lane order, waves in
//                   wave order, workgroups in the table's order -- so that equal digits keep their order (the sort is stable)
//
// Four passes of 8 bits cover the 30 code bits.  No workgroup waits on another (each step is a launch), the only atomics are integer adds and
// maxima whose results do not depend on their order, nothing is read back and nothing is allocated.  Included by gdc_kernels.hip only.
#pragma once

namespace gdc {

constexpr int RADIX_BITS = 8;
constexpr int RADIX = 1 << RADIX_BITS;
constexpr int PASSES = 4;
constexpr int CODE_BITS = 30;
static_assert(RADIX == BLOCK, "thread d of a workgroup owns digit d");
static_assert(PASSES * RADIX_BITS >= CODE_BITS, "the passes have to cover the code");
// the head of the order workspace, in 4-byte words: box[6] (~min x, y, z | max x, y, z, encoded; two words of padding) | totals[PASSES][RADIX]
constexpr int ORD_BOX = 8;
constexpr int ORD_HEAD = ORD_BOX + PASSES * RADIX;

// floats as unsigned integers of the same order (-inf < ... < -0 < +0 < ... < +inf), and back
__device__ __forceinline__ unsigned ord_enc(float x)
{
    const unsigned u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ord_dec(unsigned e) { return __uint_as_float(e ^ ((e >> 31) ? 0x80000000u : 0xffffffffu)); }

// the position a splat is ordered by: xyz, or centre[binding] + 1e-3f * xyz in fp32 (a multiply and an add, each rounded: -ffp-contract=off);
// a binding outside [0, F) reads no centre and uses (0, 0, 0)
__device__ __forceinline__ void ord_position(int i, int F, const float* __restrict__ xyz, const void* __restrict__ binding, int is64,
                                             const float* __restrict__ centers, float p[3])
{
    float c[3] = {0.f, 0.f, 0.f};
    if (centers) {   // (the face compared as 64 bits: an int64 binding such as 2^32 + 3 is outside [0, F), not face 3)
        const long long f = is64 ? reinterpret_cast<const long long*>(binding)[i] : (long long)reinterpret_cast<const int*>(binding)[i];
        if (f >= 0 && f < (long long)F)
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = centers[3 * (size_t)f + j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float x = xyz[3 * (size_t)i + j];
        p[j] = centers ? c[j] + 1e-3f * x : x;
    }
}

__global__ __launch_bounds__(BLOCK) void k_ord_clear(int* __restrict__ head)
{
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < ORD_HEAD) head[i] = 0;
}

__global__ __launch_bounds__(BLOCK) void k_ord_bounds(int P, int F, const float* __restrict__ xyz, const void* __restrict__ binding, int is64,
                                                      const float* __restrict__ centers, unsigned* __restrict__ box)
{
    __shared__ unsigned part[WAVES][6];
    const int tid = (int)threadIdx.x;
    const int i = (int)(blockIdx.x * BLOCK) + tid;
    unsigned v[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // 0 is the identity of max: box[] starts there, and the minimum is kept as the maximum of ~code
    if (i < P) {
        float p[3];
        ord_position(i, F, xyz, binding, is64, centers, p);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned e = ord_enc(p[j]);
            v[j] = ~e, v[3 + j] = e;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)v[k], d);
            v[k] = o > v[k] ? o : v[k];
        }
        if ((tid & 63) == 0) part[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < 6) {
        unsigned m = part[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) m = part[w][tid] > m ? part[w][tid] : m;
        atomicMax(&box[tid], m);
    }
}

// bit b of a 10-bit q to bit 3 b
__device__ __forceinline__ unsigned ord_spread(unsigned q)
{
    q = (q | (q << 16)) & 0x030000ffu;
    q = (q | (q << 8)) & 0x0300f00fu;
    q = (q | (q << 4)) & 0x030c30c3u;
    q = (q | (q << 2)) & 0x09249249u;
    return q;
}

__global__ __launch_bounds__(BLOCK) void k_ord_codes(int P, int F, const float* __restrict__ xyz, const void* __restrict__ binding, int is64,
                                                     const float* __restrict__ centers, const unsigned* __restrict__ box,
                                                     unsigned* __restrict__ keys)
{
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= P) return;
    float p[3];
    ord_position(i, F, xyz, binding, is64, centers, p);
    unsigned code = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double lo = (double)ord_dec(~box[j]), hi = (double)ord_dec(box[3 + j]);
        const double span = hi - lo;
        const double t = ((double)p[j] - lo) / (span > 1e-30 ? span : 1e-30) * 1023.0;   // numpy's order: subtract, divide, multiply
        // clamped BEFORE the conversion: a NaN fails the first comparison and becomes 0, +inf becomes 1023
        const unsigned q = t >= 0.0 ? (t < 1023.0 ? (unsigned)t : 1023u) : 0u;
        code |= ord_spread(q) << j;
    }
    keys[i] = code;
}

__global__ __launch_bounds__(BLOCK) void k_ord_hist(int P, int nchunks, int shift, const unsigned* __restrict__ keys, int* __restrict__ table,
                                                    int* __restrict__ totals)
{
    __shared__ int hist[RADIX];
    const int tid = (int)threadIdx.x;
    const int i = (int)(blockIdx.x * BLOCK) + tid;
    hist[tid] = 0;
    __syncthreads();
    if (i < P) atomicAdd(&hist[(keys[i] >> shift) & (RADIX - 1)], 1);
    __syncthreads();
    const int n = hist[tid];
    table[(size_t)tid * nchunks + blockIdx.x] = n;
    if (n) atomicAdd(&totals[tid], n);
}

// workgroup d: row d of the table -> the exclusive prefix over the workgroups, starting at the number of keys with a smaller digit
__global__ __launch_bounds__(BLOCK) void k_ord_scan(int nchunks, int* __restrict__ table, const int* __restrict__ totals)
{
    __shared__ int lane_sum[BLOCK];
    __shared__ int below[WAVES];
    const int tid = (int)threadIdx.x, digit = (int)blockIdx.x;
    int* __restrict__ row = table + (size_t)digit * nchunks;
    int b = tid < digit ? totals[tid] : 0;
    for (int d = 32; d > 0; d >>= 1) b += __shfl_xor(b, d);
    if ((tid & 63) == 0) below[tid >> 6] = b;
    const int per = (nchunks + BLOCK - 1) / BLOCK;
    const int lo = tid * per < nchunks ? tid * per : nchunks;
    const int hi = lo + per < nchunks ? lo + per : nchunks;
    int mine = 0;
    for (int c = lo; c < hi; ++c) mine += row[c];
    lane_sum[tid] = mine;
    __syncthreads();
    for (int d = 1; d < BLOCK; d <<= 1) {   // inclusive scan over the 256 threads
        const int add = tid >= d ? lane_sum[tid - d] : 0;
        __syncthreads();
        lane_sum[tid] += add;
        __syncthreads();
    }
    int run = lane_sum[tid] - mine;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) run += below[w];
    for (int c = lo; c < hi; ++c) {
        const int v = row[c];
        row[c] = run;
        run += v;
    }
}

// vals NULL: the value of key i is i (the first pass); keys_out NULL: the keys are not needed again (the last pass)
__global__ __launch_bounds__(BLOCK) void k_ord_scatter(int P, int nchunks, int shift, const unsigned* __restrict__ keys,
                                                       const int* __restrict__ vals, const int* __restrict__ table,
                                                       unsigned* __restrict__ keys_out, int* __restrict__ vals_out)
{
    __shared__ int count[WAVES][RADIX];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = (int)(blockIdx.x * BLOCK) + tid;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) count[w][tid] = 0;
    __syncthreads();
    const bool live = i < P;
    const unsigned key = live ? keys[i] : 0u;
    const int digit = (int)((key >> shift) & (RADIX - 1));
    unsigned long long peers = __ballot(live);   // the live lanes of this wave with this lane's digit
#pragma unroll
    for (int b = 0; b < RADIX_BITS; ++b) {
        const unsigned long long m = __ballot((digit >> b) & 1);
        peers &= ((digit >> b) & 1) ? m : ~m;
    }
    const int before = __popcll(peers & ((1ull << lane) - 1ull));
    if (live && before == 0) count[wave][digit] = __popcll(peers);
    __syncthreads();
    if (!live) return;
    int pos = table[(size_t)digit * nchunks + blockIdx.x] + before;
    for (int w = 0; w < wave; ++w) pos += count[w][digit];
    if ((unsigned)pos >= (unsigned)P) return;   // (a table the three steps made never gets here: nothing is ever stored out of range)
    if (keys_out) keys_out[pos] = key;
    vals_out[pos] = vals ? vals[i] : i;
}

// the order workspace: head[ORD_HEAD] | keys[2][P] | vals[2][P] | table[RADIX * nchunks]
struct OrderWorkspace { unsigned* box; int* totals; unsigned* keys[2]; int* vals[2]; int* table; int nchunks; };

static OrderWorkspace carve_order(void* base, int P)
{
    OrderWorkspace w;
    w.nchunks = (P + BLOCK - 1) / BLOCK;
    w.box = (unsigned*)base;
    w.totals = (int*)base + ORD_BOX;
    w.keys[0] = (unsigned*)base + ORD_HEAD;
    w.keys[1] = w.keys[0] + P;
    w.vals[0] = (int*)(w.keys[1] + P);
    w.vals[1] = w.vals[0] + P;
    w.table = w.vals[1] + P;
    return w;
}

}  // namespace gdc

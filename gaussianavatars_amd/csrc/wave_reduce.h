// wave_reduce.h -- the wave64 reductions on the DPP network (gfx950), once for every library: libgsr takes them through gsr_device.h,
// gab, gls and gev include this directly.  Device code only, all of it __forceinline__: every translation unit compiles it under its own
// -ffp-contract setting (nothing here can contract: the sums are plain adds).
// The __shfl_xor / __shfl_down loops of grl, gdc and three gsr kernels are NOT these: their float summation order differs from the tree
// below, so they stay where they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wave_reduce {

// ---- wave64 reductions on the DPP network -------------------------------------------------
// xor-butterfly inside each 16-lane row (quad_perm, row_half_mirror, row_mirror), then
// row_bcast:15 into rows 1,3 and row_bcast:31 into rows 2,3: lanes 48..63 end up holding the
// full 64-lane sum.
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
__device__ __forceinline__ float wave_sum_hi(float v)
{
    v += dpp_f<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
    v += dpp_f<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
    v += dpp_f<0x141, 0xf>(v);  // row_half_mirror
    v += dpp_f<0x140, 0xf>(v);  // row_mirror
    v += dpp_f<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3
    v += dpp_f<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3
    return v;                   // valid in lanes 48..63
}
__device__ __forceinline__ double wave_sum_hi(double v)   // the same tree in fp64
{
    v += dpp_d<0xB1, 0xf>(v);
    v += dpp_d<0x4E, 0xf>(v);
    v += dpp_d<0x141, 0xf>(v);
    v += dpp_d<0x140, 0xf>(v);
    v += dpp_d<0x142, 0xa>(v);
    v += dpp_d<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
    // ds_swizzle-free max: butterfly through readlane-able DPP moves
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false));
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false));
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false));
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false));
    uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
    uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return mx(mx(a, b), mx(c, d));
}

// inclusive prefix sum across the 64 lanes in six DPP adds (row_shr inside the rows of 16, then the row totals broadcast to the
// rows above): no LDS crossbar round trips (ds_bpermute), which is what __shfl_up costs per step
__device__ __forceinline__ uint32_t wave_scan_incl_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}

}  // namespace wave_reduce

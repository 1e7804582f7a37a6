/*
 * glp.h -- C ABI of the LPIPS evaluation metric ("Gaussian LPIPS"): lpipsPyTorch's forward (lpipsPyTorch/__init__.py,
 * modules/{lpips,networks,utils}.py) for the `alex` and `vgg` backbones, as a small fixed forward-only convolutional
 * network on fp32-input MFMA.
 *
 *   glp_pack_weights   a (Cout,Cin,k,k) convolution weight into the K-major layout glp_conv2d reads, once per loaded model
 *   glp_conv2d         direct convolution as an implicit GEMM: the im2col gather goes to LDS only, bias and ReLU in the epilogue
 *   glp_maxpool        k3 s2 / k2 s2 max pooling, floor mode, no padding
 *   glp_zscore         (x - mean) / std per channel of BOTH images, into one batch of 2B
 *   glp_head           one tap: channel norms (eps outside the square root), (fx/|fx| - fy/|fy|)^2, the tap's 1x1 weights, the
 *                      spatial and batch sum as per-workgroup partials
 *   glp_finish         the five taps' partials -> five terms and their sum
 *   glp_forward        the whole chain of one net on one pair of batches, every launch above enqueued by one call
 *
 * Conventions as gev.h: DEVICE pointers, contiguous fp32 NCHW buffers; 0 / <0 return codes with glp_last_error();
 * everything is enqueued on `stream`, nothing synchronises and nothing is read back.  Reductions run in a fixed order
 * with no float atomics: a result is the same bits run to run.  Every entry is evaluation-only (there is no backward).
 * Arithmetic is fp32 throughout (the MFMA is the f32-input one: a k-ordered fmaf chain); only the head's partials and the
 * finishing sum are fp64.
 */
#ifndef GLP_H
#define GLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLP_ABI_VERSION 1
#define GLP_OK 0
#define GLP_E_ARG (-1)
#define GLP_E_HIP (-2)

#define GLP_NET_ALEX 0
#define GLP_NET_VGG 1
#define GLP_TAPS 5          /* taps of either net */
#define GLP_MAX_CONVS 13    /* convolutions of the larger net (vgg); alex has 5 */
#define GLP_TILE 64         /* output channels and output pixels per workgroup of glp_conv2d: Cout must be a multiple */
#define GLP_KBLOCK 16       /* reduction elements per LDS stage: packed weights are zero-padded to a multiple */
#define GLP_HEAD_BLOCKS 256 /* most workgroups (= partials) of one glp_head launch */
#define GLP_OUT_FLOATS 6    /* glp_finish / glp_forward: the five per-tap terms, then their sum */

int glp_abi_version(void);
const char* glp_last_error(void);

/* number of convolutions of a net (5 / 13), or < 0 */
int glp_net_convs(int32_t net);

/* floats of the packed form of a (Cout,Cin,k,k) weight: Cout * (Cin*k*k rounded up to GLP_KBLOCK); < 0 on a bad shape */
int64_t glp_packed_floats(int32_t Cin, int32_t Cout, int32_t k);
/* packed[kk * Cout + co] <- w[co][kk] for kk = (c*k + ky)*k + kx < Cin*k*k, and 0 for the padding rows.  One launch. */
int glp_pack_weights(int32_t Cin, int32_t Cout, int32_t k, const float* w, float* packed, void* stream);

/* out (N,Cout,Ho,Wo) <- conv(x (N,Cin,H,W), w) + bias, then max(., 0) when relu != 0;  Ho = (H + 2*pad - k) / stride + 1, likewise Wo.
 * k in {1,3,5,11}, stride >= 1, 0 <= pad < k, Cout a multiple of GLP_TILE, zero padding.  `packed` is glp_pack_weights' output, bias
 * is Cout floats or NULL.  A workgroup forms GLP_TILE channels of GLP_TILE output pixels (pixels run across images); the reduction over
 * K = Cin*k*k runs in blocks of GLP_KBLOCK on v_mfma_f32_16x16x4_f32, its four k-steps in four accumulators added pairwise at the end.
 * One launch.  out must not alias x. */
int glp_conv2d(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t k, int32_t stride, int32_t pad, const float* x,
               const float* packed, const float* bias, int32_t relu, float* out, void* stream);

/* out (planes,Ho,Wo) <- max over k x k windows of x (planes,H,W) at `stride`;  Ho = (H - k) / stride + 1 (floor mode, no padding).
 * (k, stride) is (3,2) or (2,2).  The values are x's own (bit-equal to torch.nn.functional.max_pool2d).  One launch. */
int glp_maxpool(int64_t planes, int32_t H, int32_t W, int32_t k, int32_t stride, const float* x, float* out, void* stream);

/* out (2B,3,H,W) <- (x - mean[c]) / std[c] for images 0..B-1, the same of y for images B..2B-1;
 * mean = (-.030, -.088, -.188), std = (.458, .448, .450).  One launch. */
int glp_zscore(int32_t B, int32_t H, int32_t W, const float* x, const float* y, float* out, void* stream);

/* workgroups (= doubles of `partial`) one glp_head launch over B pairs of H x W positions uses: min(GLP_HEAD_BLOCKS, ceil(B*H*W / 256)) */
int32_t glp_head_blocks(int32_t B, int32_t H, int32_t W);
/* feat (2B,C,H,W): images 0..B-1 are x's features, B..2B-1 are y's.  For every pair b and position p:
 *   nx = sqrt(sum_c fx^2) + 1e-10,  ny likewise,  s(b,p) = sum_c lin[c] * (fx/nx - fy/ny)^2      (fp32, c ascending)
 * and partial[g] <- the fp64 sum of the s(b,p) workgroup g owns, added in a fixed order.  An all-zero position contributes 0, never a NaN;
 * an identical pair contributes exactly 0.  One launch. */
int glp_head(int32_t B, int32_t C, int32_t H, int32_t W, const float* feat, const float* lin, double* partial, void* stream);

/* out[t] <- (sum of the first blocks[t] doubles of partial + t * GLP_HEAD_BLOCKS) / hw[t] for t < GLP_TAPS, out[GLP_TAPS] <- their sum (in
 * fp64, rounded once): lpips.py:33-36, the sum over taps AND over the batch.  blocks and hw are HOST arrays of GLP_TAPS.  One launch of one
 * workgroup. */
int glp_finish(const double* partial, const int32_t* blocks, const int32_t* hw, float* out, void* stream);

/* bytes of workspace glp_forward needs for B pairs of 3 x H x W images: two activation buffers of the largest layer, and the
 * head partials.  < 0 when the net is unknown or the image is too small for the net's strides and pools. */
int64_t glp_workspace_bytes(int32_t net, int32_t B, int32_t H, int32_t W);

/* The whole metric on x, y (B,3,H,W): z-score, every convolution and pool of the net up to its last tap, a head launch after each tap's
 * ReLU, and the finishing launch.  conv_w / conv_b / lin are HOST arrays of device pointers: the glp_net_convs(net) packed weights and
 * biases in layer order, and the GLP_TAPS 1x1 weights.  out: GLP_OUT_FLOATS floats.  workspace: glp_workspace_bytes, 16-byte aligned.
 * alex: 1 + 5 + 2 + 5 + 1 = 14 launches, vgg: 1 + 13 + 4 + 5 + 1 = 24. */
int glp_forward(int32_t net, int32_t B, int32_t H, int32_t W, const float* x, const float* y, const void* const* conv_w,
                const void* const* conv_b, const void* const* lin, void* workspace, float* out, void* stream);

/* Optional per-kernel timing with hipEvents on the launch stream, as gls_profile_* (include/gls.h). */
int glp_profile_enable(int on);
int glp_profile_collect(void);
int glp_profile_entry(int32_t index, const char** name, double* total_ms, int64_t* launches);
int glp_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GLP_H */

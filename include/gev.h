/*
 * gev.h -- C ABI of the evaluation and export passes ("Gaussian evaluation"): what the reference does with a
 * rendered image outside the training step.
 *
 *   gev_pair_stats / gev_accumulate   train.py:256-309 (training_report: two clamps, l1_loss, psnr, ssim, three
 *                            running sums) and metrics.py:67-74 (ssim and psnr of the decoded PNG pair): ONE pass
 *                            over an image pair yields, per plane, sum |a-b|, sum (a-b)^2 and the sum of the SSIM
 *                            map (utils/loss_utils.py:36-63: 11x11 Gaussian window sigma 1.5, zero padding,
 *                            C1 = 0.01^2, C2 = 0.03^2); the reducing launch forms the image's L1 / PSNR / SSIM from
 *                            them (utils/image_utils.py:18-20) and adds them to running sums that stay on the device.
 *   gev_to_u8                render.py:41, `data.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)`: the
 *                            bytes of the image file, in one launch.
 *
 * Conventions as gls.h: DEVICE pointers, contiguous buffers; 0 / <0 return codes with gev_last_error(); everything
 * is enqueued on `stream`, nothing synchronises and nothing is read back.  Reductions run in a fixed order with no
 * float atomics: a result is the same bits run to run.  Every entry is evaluation-only (there is no backward).
 */
#ifndef GEV_H
#define GEV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEV_ABI_VERSION 1
#define GEV_OK 0
#define GEV_E_ARG (-1)
#define GEV_E_HIP (-2)
#define GEV_SSIM_WINDOW 11

/* layout of one image of a pair */
#define GEV_F32_PLANAR 0       /* float (B,C,H,W): what render() returns */
#define GEV_U8_INTERLEAVED 1   /* uint8 (B,H,W,C): what a decoded PNG is; always read as byte / 255.f (torchvision's to_tensor) */

/* load transform of a GEV_F32_PLANAR image, applied ONCE to every pixel as it is read; all three statistics are taken over the
 * transformed values */
#define GEV_RAW 0     /* none */
#define GEV_CLAMP 1   /* min(max(x, 0), 1): train.py:277-278 */
#define GEV_PNG8 2    /* the byte gev_to_u8 writes for x, divided by 255 in fp32: what metrics.py sees after the PNG round trip */

/* how gev_accumulate forms an image's PSNR from its planes (utils/image_utils.py:18-20 takes the mean over view(shape[0], -1)) */
#define GEV_PSNR_PER_CHANNEL 0   /* 20 log10(1 / sqrt(mse)) of every plane, then their mean: psnr((3,H,W)).mean() of training_report */
#define GEV_PSNR_PER_IMAGE 1     /* one mse over the C planes of the image: psnr((1,3,H,W)) of metrics.py */

int gev_abi_version(void);
const char* gev_last_error(void);

/* floats of scratch (`partial`, 8-byte aligned) the two statistics entries need for B images of C x H x W */
int64_t gev_partial_floats(int32_t B, int32_t C, int32_t H, int32_t W);

/* a, b: B images of C x H x W in the layouts a_layout, b_layout; `transform` applies to the GEV_F32_PLANAR ones.
 * plane_sums: (B*C, 3) DOUBLES <- { sum |a-b|, sum (a-b)^2, sum ssim_map } of every plane.  |a-b| and the SSIM map are fp32 values summed
 * per 32x16 tile in fp32 (the arithmetic of gls_l1_ssim_forward: separable taps added in the order k = 0..10); (a-b)^2 is formed and summed
 * in fp64; the tiles of a plane are added in fp64.  Two launches; the second is ONE workgroup (B*C planes, four at a time).
 * B*C <= 65535.  Non-finite pixels are out of contract (they do not fault). */
int gev_pair_stats(int32_t B, int32_t C, int32_t H, int32_t W, const void* a, int32_t a_layout, const void* b, int32_t b_layout,
                   int32_t transform, double* plane_sums, float* partial, void* stream);

/* gev_pair_stats, and inside its reducing launch (still two launches per pair) the figures of every image i of the B:
 *   l1 = sum_c sum|a-b| / (C*H*W),  psnr per `psnr_mode` (+inf for an identical pair, as the reference),  ssim = sum_c sum ssim_map / (C*H*W)
 * formed in fp64, rounded to fp32 and
 *   per_view[(row + i) * 3 + {0,1,2}] <- { l1, psnr, ssim }                          (fp32 table of at least row + B rows, or NULL)
 *   acc[0..2] += (double) of those fp32 values,  acc[3] += 1                          (4 DOUBLES [l1, psnr, ssim, count], or NULL)
 * -- the reference's `.mean().double()` followed by `+=` (train.py:286-288).  Nothing is read back: an evaluation of N views reads acc once. */
int gev_accumulate(int32_t B, int32_t C, int32_t H, int32_t W, const void* a, int32_t a_layout, const void* b, int32_t b_layout,
                   int32_t transform, int32_t psnr_mode, double* plane_sums, float* partial, float* per_view, int32_t row, double* acc,
                   void* stream);

/* src: float (B,C,H,W) -> dst: uint8 (B,H,W,C) with exactly the roundings of render.py:41: ONE fp32 multiply by 255, ONE fp32 add of 0.5
 * (never fused), clamp to [0, 255], truncation.  src2 / dst2: a second image of the same shape converted by the same launch (the ground truth
 * render.py:85 writes beside every render), or both NULL.  GEV_PNG8 above is this very device function.  One launch; 16-byte loads per plane
 * and packed stores when C == 3, H*W is a multiple of 4 and the buffers are 16-byte aligned.  Non-finite inputs are out of contract: they do
 * not fault (a NaN becomes 0, torch leaves it undefined). */
int gev_to_u8(int32_t B, int32_t C, int32_t H, int32_t W, const float* src, uint8_t* dst, const float* src2, uint8_t* dst2, void* stream);

/* Optional per-kernel timing with hipEvents on the launch stream, as gls_profile_* (include/gls.h). */
int gev_profile_enable(int on);
int gev_profile_collect(void);
int gev_profile_entry(int32_t index, const char** name, double* total_ms, int64_t* launches);
int gev_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GEV_H */

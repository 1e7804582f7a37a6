/*
 * gfs.h -- C ABI of the resident frame store ("Gaussian frame store"): the training frames of a subject kept in HBM
 * as the 8-bit images they are, and the two passes that move them.
 *
 *   gfs_compose        scene/__init__.py:48-51 (CameraDataset.__getitem__): the decoded RGBA bytes composited over
 *                      the camera's background in fp64 and quantised back to bytes, once per frame, at ingest.
 *   gfs_resample       scene/__init__.py:54 (PILtoTorch's `pil_image.resize(resolution)`) for a camera that asks for another size than
 *                      its file's (--resolution 2/4/8, -r WIDTH, the rescale of images wider than 1600 px): Pillow's bicubic resize
 *                      of the composited bytes, byte for byte, once per frame, at ingest.
 *   gfs_fetch*         scene/__init__.py:54-62 (PILtoTorch at the file's own size, [:3], clamp): one stored frame as
 *                      the planar fp32 (3,H,W) `original_image` train.py:128 uploads, in one launch.
 *
 * The store of one (H, W) group is `capacity` frames of gfs_frame_stride(H, W) bytes each: RGB interleaved, H*W*3
 * bytes, then padding.  The stride is a multiple of 16 and covers whole groups of four pixels, so every frame base is
 * 16-byte aligned and a lane's three dword loads never leave its frame.
 *
 * Conventions as gev.h: DEVICE pointers unless said otherwise, contiguous buffers; 0 / <0 return codes with
 * gfs_last_error(); everything is enqueued on `stream`, nothing synchronises and nothing is read back.  All byte
 * offsets are 64-bit: a store may be larger than 4 GiB.
 */
#ifndef GFS_H
#define GFS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFS_ABI_VERSION 2
#define GFS_OK 0
#define GFS_E_ARG (-1)
#define GFS_E_HIP (-2)
#define GFS_E_RANGE (-3)        /* a HOST index outside [0, count) */
#define GFS_TABLE_ENTRIES 256   /* floats of the byte-to-float table */
#define GFS_MAX_BATCH 65535     /* frames one gfs_fetch_batch or gfs_compose launch takes */
#define GFS_FLAG_RANGE 1        /* bit set in *flag when a DEVICE index was outside [0, count) */

int gfs_abi_version(void);
const char* gfs_last_error(void);

/* bytes from one stored frame of H x W to the next: 12 * ceil(H*W / 4) rounded up to a multiple of 16; 0 for a bad shape */
int64_t gfs_frame_stride(int32_t H, int32_t W);

/* rgba: `count` images (H,W,4) uint8, contiguous -> frames first .. first + count - 1 of `store` (capacity frames).
 * bg: three HOST doubles.  Per pixel and channel, all in fp64 and in the reference's order, nothing fused:
 *   n = byte / 255.0;  arr = n_rgb * n_a + bg * (1 - n_a);  v = arr * 255.0;  stored byte = low 8 bits of (int)v (truncation toward zero)
 * -- `np.array(arr * 255.0, dtype=np.byte)` reinterpreted as "RGB".  The bytes of a frame's last group of four behind its last pixel are written as zeros.
 * One launch; a lane takes four pixels (one 16-byte load where the source allows, three dword stores). */
int gfs_compose(int32_t H, int32_t W, const uint8_t* rgba, const double* bg, uint8_t* store, int64_t capacity, int64_t first, int32_t count,
                void* stream);

/* `PIL.Image.resize((Wout, Hout))` with its defaults (bicubic, no reducing_gap) of `count` stored "RGB" frames: frames src_first .. of `src`
 * (a store of src_capacity frames of Hin x Win) -> frames first .. first + count - 1 of `store` (capacity frames of Hout x Wout).  The two
 * stores must not overlap.  Pillow's passes, in its order: the horizontal axis, bytes, the vertical axis; an axis whose size does not
 * change is skipped.  Per axis and output index i, with the HOST-computed tables of that axis (DEVICE pointers; frames.resample_tables):
 *   k: int32 (out, ks), the weights of Resample.c's precompute_coeffs in fp64, normalised, times 2^22, rounded half away from zero
 *   b: int32 (out, 2), (first source index, taps); a kernel holds them to the axis and to ks, and they must not decrease with i
 *   byte = clamp((2^21 + sum_{t < taps} source_byte[first + t] * k[i][t]) >> 22, 0, 255)       (int32 sum, arithmetic shift)
 * The coefficients are not formed here: this translation unit multiplies bytes by integers and nothing else, so no contraction or
 * reassociation can move a last bit.  kx / bx are null exactly when Win == Wout, ky / by exactly when Hin == Hout; at least one axis changes.
 * tmp: gfs_resample_tmp_bytes(Hin, Wout, count) bytes, 16-byte aligned, needed (and touched) only when both axes change.
 * Every byte of a destination frame's stride behind its last pixel is written as zero.  One launch per pass, each over all `count` frames. */
int64_t gfs_resample_tmp_bytes(int32_t Hin, int32_t Wout, int32_t count);   /* 0 for a bad shape or count */
int gfs_resample(int32_t Hin, int32_t Win, const uint8_t* src, int64_t src_capacity, int64_t src_first, int32_t Hout, int32_t Wout,
                 const int32_t* kx, const int32_t* bx, int32_t ksx, const int32_t* ky, const int32_t* by, int32_t ksy, uint8_t* tmp, uint8_t* store,
                 int64_t capacity, int64_t first, int32_t count, void* stream);

/* frame `index` (HOST value; GFS_E_RANGE outside [0, count)) of `store` -> out: float (3,H,W), out[c][y][x] = table[byte].
 * table: GFS_TABLE_ENTRIES floats, `torch.arange(256, dtype=uint8) / 255.0` computed by the caller: the kernel stages it in LDS and never
 * divides, so the floats are torch's bits.  One launch; a lane takes four pixels: three dword loads, one 16-byte store per plane when H*W
 * is a multiple of 4 and `out` is 16-byte aligned, scalar stores (and a guarded tail) otherwise. */
int gfs_fetch(int32_t H, int32_t W, const uint8_t* store, int64_t count, int64_t index, const float* table, float* out, void* stream);

/* gfs_fetch with the index read from DEVICE memory (one int64) inside the kernel: no host read, so the call can be captured in a graph and
 * replayed with another index.  An index outside [0, count) writes nothing to `out` and ORs GFS_FLAG_RANGE into *flag (int32, caller-zeroed). */
int gfs_fetch_indexed(int32_t H, int32_t W, const uint8_t* store, int64_t count, const int64_t* index, const float* table, float* out,
                      int32_t* flag, void* stream);

/* K frames by a DEVICE list of K int64 indices -> out: float (K,3,H,W), in one launch.  An index outside [0, count) leaves its image
 * unwritten and ORs GFS_FLAG_RANGE into *flag.  K <= GFS_MAX_BATCH. */
int gfs_fetch_batch(int32_t H, int32_t W, const uint8_t* store, int64_t count, const int64_t* indices, int32_t K, const float* table, float* out,
                    int32_t* flag, void* stream);

/* Optional per-kernel timing with hipEvents on the launch stream, as gls_profile_* (include/gls.h). */
int gfs_profile_enable(int on);
int gfs_profile_collect(void);
int gfs_profile_entry(int32_t index, const char** name, double* total_ms, int64_t* launches);
int gfs_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* GFS_H */

/* static_clip_ops_hip.h -- C ABI of libstatic_clip_ops_hip.so: a training clip made from ONE still image, the
 * reference's MultiRandomShift (data/transforms.py:173-223), as one gfx950 kernel launch per clip.
 *
 * The definition ("Static-image clips") is integer arithmetic on a table the CALLER builds, Pillow's 8-bit
 * resample of hc samples to h (memotr_amd.data.augment.resample_tables(hc, h)):
 *   per output row y:  xmin[y] first source row, cnt[y] taps, kk[y * ksize + j] weight of tap j in 1/2**22
 *                      (j < cnt[y] <= ksize; non-negative, summing to about 2**22, so the sums below fit int32)
 *   p_0 = the h x w source image seen through `flip` (column x of p_0 is image column w - 1 - x) and `swap_rb`
 *         (channel c of p_0 is image channel 2 - c)
 *   p_k(y, x, c) = clamp((2**21 + sum_{j < cnt[y]} p_{k-1}(y0 + xmin[y] + j, x + s, c) * kk[y][j]) >> 22, 0, 255)
 *         with p_{k-1}(., x', .) = 0 for x' >= w                                      k = 1 .. T - 1
 *   out[k * out_frame_pitch + y * out_row_pitch + 3 * x + c] = p_k(y, x, c)            k = 0 .. T - 1
 * Column x of frame k is the vertical pass applied k times to column x + k * s of p_0, or black once x + k * s >= w:
 * the chain is column-parallel, and every byte of the T frames is written, frame 0 and the black columns included.
 *
 * All pointers are device pointers, sizes are plain integers, nothing is kept between calls except the text of the
 * last error of the calling thread (no call changes the meaning of a later one).  Returns 0 on success or a non-zero
 * code (staticclip_last_error() has the text); launches on `stream` (a hipStream_t passed as void*; NULL = the default
 * stream) and does not synchronise.  Arguments are validated on the host, without touching a device.
 */
#ifndef STATIC_CLIP_OPS_HIP_H
#define STATIC_CLIP_OPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STATICCLIP_ABI_VERSION 1

int staticclip_abi_version(void);
const char *staticclip_last_error(void);

/* The launch plan of an h x w image, decided from h and w alone (host only, no device is touched):
 *   *strip      source columns one workgroup owns;
 *   *lds_bytes  LDS of one workgroup: two images of h rows of the strip, or 0 when h is too tall for that and the
 *               workgroup keeps the chain in the output frames themselves (global memory; same arithmetic).
 * Returns 0, or non-zero for a null pointer or a non-positive size. */
int staticclip_plan(int h, int w, int *strip, int *lds_bytes);

/* src: h rows of w pixels of 3 bytes; byte (y, x, c) at src[y * row_pitch + 3 * x + c] (row_pitch >= 3 * w; any
 *      alignment: rows need not start on a dword).
 * T >= 1 frames; s >= 0 columns and the row window y0 .. y0 + hc - 1 (y0 >= 0, hc >= 1, y0 + hc <= h) of the previous
 *      frame that the next one is made of.  s >= w makes every derived frame black.
 * xmin, cnt (h) and kk (h * ksize): int32, xmin >= 0, cnt >= 1, xmin + cnt <= hc.  (Tap counts are loop bounds and
 *      row indices are clamped to the image, so a table that breaks this gives wrong levels, never a read outside
 *      the image.)
 * out: T frames of h rows of w pixels, out_row_pitch >= 3 * w, any alignment; for T > 1 out_frame_pitch >=
 *      (h - 1) * out_row_pitch + 3 * w (frames do not overlap).  Bytes between rows and frames are left alone.
 *      out must not overlap src.
 * One launch covers the clip. */
int staticclip_shift_chain(const uint8_t *src, long row_pitch, int h, int w, int T, int flip, int swap_rb,
                           int s, int y0, int hc,
                           const int32_t *xmin, const int32_t *cnt, const int32_t *kk, int ksize,
                           uint8_t *out, long out_row_pitch, long out_frame_pitch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* STATIC_CLIP_OPS_HIP_H */

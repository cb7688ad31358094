/* frame_ops_hip.h -- C ABI of libframe_ops_hip.so: a decoded video frame (uint8, H x W x 3) to the padded, normalised
 * fp32 planes the model reads, as one gfx950 kernel (the reference does this on the CPU: data/seq_dataset.py:33-43,
 * cv2.resize -> to_tensor -> normalize, then utils/nested_tensor.py pads to a multiple of 32).
 *
 * The definition ("Raw-frame ingestion") is integer arithmetic on tables the CALLER builds:
 *   per destination column x:  s0x[x], s1x[x] source columns (int32), a1x[x] weight of s1x in 1/2048 (int16; a0 = 2048 - a1)
 *   per destination row    y:  s0y[y], s1y[y] source rows,             b1y[y] weight of s1y (b0 = 2048 - b1)
 *   r(row, x) = p[row][s0x] * a0 + p[row][s1x] * a1                                  (p: source level of one channel)
 *   q = ( ((b0 * (r(s0y, x) >> 4)) >> 16) + ((b1 * (r(s1y, x) >> 4)) >> 16) + 2 ) >> 2          (a level 0..255)
 *   out[b][c][y][x] = lut[c * 256 + q]   for y < th and x < tw,   0.0f elsewhere (the padding, written in the same pass)
 * with c the OUTPUT channel; it reads source channel c, or 2 - c when `swap_rb` is set (BGR frames).
 *
 * All pointers are device pointers, sizes are plain integers, nothing is kept between calls except the text of the
 * last error of the calling thread (no call changes the meaning of a later one).  Returns 0 on success or a non-zero
 * code (frameops_last_error() has the text); launches on `stream` (a hipStream_t passed as void*; NULL = the default
 * stream) and does not synchronise.  Arguments are validated on the host, without touching a device.
 */
#ifndef FRAME_OPS_HIP_H
#define FRAME_OPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRAMEOPS_ABI_VERSION 1

int frameops_abi_version(void);
const char *frameops_last_error(void);

/* src: B frames of h rows of w pixels of 3 bytes; byte (b, y, x, c) at src[b * frame_pitch + y * row_pitch + 3 * x + c]
 *      (row_pitch >= 3 * w; any alignment: rows need not start on a dword).
 * s0x, s1x (tw) int32 in [0, w) with s0x <= s1x; a1x (tw) int16 in [0, 2048]; s0y, s1y (th) int32 in [0, h) with
 *      s0y <= s1y; all four non-decreasing in their index; b1y (th) int16 in [0, 2048].
 * lut: 3 * 256 floats, the normalised value of level q for output channel c at lut[c * 256 + q].
 * out: (B, 3, Hp, Wp) fp32 contiguous, 16-byte aligned, Hp >= th, Wp >= tw, Wp a multiple of 4; every element is written.
 * One launch covers all B frames.  B == 0 returns 0 and launches nothing. */
int frameops_resize_normalize_u8(const uint8_t *src, long row_pitch, long frame_pitch, int B, int h, int w,
                                 const int32_t *s0x, const int32_t *s1x, const int16_t *a1x, const int32_t *s0y,
                                 const int32_t *s1y, const int16_t *b1y, int th, int tw, int Hp, int Wp,
                                 const float *lut, int swap_rb, float *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRAME_OPS_HIP_H */

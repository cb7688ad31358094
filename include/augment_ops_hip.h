/* augment_ops_hip.h -- C ABI of libaugment_ops_hip.so: the pixel side of the training-clip augmentation as one gfx950
 * kernel per resize (the reference does it on the CPU: data/transforms.py, PIL bilinear resize / crop, cv2 HSV jitter,
 * to_tensor, normalize; utils/nested_tensor.py pads to a multiple of 32).
 *
 * The definition ("Training-clip augmentation") is integer arithmetic on tables the CALLER builds, Pillow's
 * 8-bit resample per axis:
 *   per output index i:  xmin[i] first source index, cnt[i] taps, kk[i * ksize + k] weight of tap k in 1/2**22
 *                        (k < cnt[i] <= ksize; non-negative, summing to about 2**22, so the sums below fit int32)
 *   m(row, x, c) = clamp((2**21 + sum_k p[row][xmin_x[x] + k][c] * kk_x[x][k]) >> 22, 0, 255)     horizontal, to bytes
 *   q(y, x, c)   = clamp((2**21 + sum_k m(xmin_y[y] + k, x, c) * kk_y[y][k]) >> 22, 0, 255)       vertical
 * where p is the h x w source window seen through `flip` (column x of p is window column w - 1 - x) and `swap_rb`
 * (channel c of p is window channel 2 - c).  The tables may be slices of a larger resize's tables: that resize followed
 * by a crop.  Then one of two output stages:
 *   AUGOPS_STAGE_U8   out_u8[t * out_frame_pitch + y * out_row_pitch + 3 * x + c] = q
 *   AUGOPS_STAGE_F32  (r, g, b) = q, through the HSV jitter if use_hsv:
 *                       v = max, d = v - min, s = (d * sdiv[v] + 2048) >> 12,
 *                       h0 = g - b if v == r, else b - r + 2d if v == g, else r - g + 4d,
 *                       h = (h0 * hdiv[d] + 2048) >> 12 (arithmetic shift), + 180 if negative;
 *                       h = (h + dh) mod 180 (non-negative), s = clamp(s + ds, 0, 255), v = clamp(v + dv, 0, 255);
 *                       sec = h / 30, f = h % 30, D = 7650, p = (v * (255 - s) * 30 + D/2) / D,
 *                       q = (v * (D - s * f) + D/2) / D, t = (v * (D - s * (30 - f)) + D/2) / D,
 *                       (r, g, b) = (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q) for sec 0..5;
 *                     out_f32[t'][c][y][x] = lut[c * 256 + level of channel c] for y < oh and x < ow, 0.0f elsewhere
 *                     (the padding, written in the same pass); t' = T - 1 - t if `reverse`, else t.
 *
 * All pointers are device pointers, sizes are plain integers, nothing is kept between calls except the text of the
 * last error of the calling thread (no call changes the meaning of a later one).  Returns 0 on success or a non-zero
 * code (augops_last_error() has the text); launches on `stream` (a hipStream_t passed as void*; NULL = the default
 * stream) and does not synchronise.  Arguments are validated on the host, without touching a device.
 */
#ifndef AUGMENT_OPS_HIP_H
#define AUGMENT_OPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUGOPS_ABI_VERSION 1
#define AUGOPS_STAGE_U8 0
#define AUGOPS_STAGE_F32 1

int augops_abi_version(void);
const char *augops_last_error(void);

/* src: T windows of h rows of w pixels of 3 bytes; byte (t, y, x, c) at src[t * frame_pitch + y * row_pitch + 3 * x + c]
 *      (row_pitch >= 3 * w; any alignment: rows need not start on a dword).
 * xmin_x, cnt_x (ow) and kk_x (ow * ksize_x), xmin_y, cnt_y (oh) and kk_y (oh * ksize_y): int32, xmin >= 0,
 *      cnt >= 1, xmin + cnt <= w (h), xmin and xmin + cnt non-decreasing in the index.  (Indices are clamped to the
 *      window, so a table that breaks this gives wrong levels, never a read outside the window.)
 * AUGOPS_STAGE_U8:  out_u8 with out_row_pitch >= 3 * ow, any alignment; the f32 arguments are ignored.
 * AUGOPS_STAGE_F32: out_f32 (T, 3, Hp, Wp) fp32 contiguous, 16-byte aligned, Hp >= oh, Wp >= ow, Wp a multiple of 4,
 *      every element is written; lut: 3 * 256 floats; use_hsv 0 / 1; hsv_div: 2 * 256 int32 (sdiv, then hdiv), needed
 *      if use_hsv; |dh|, |ds|, |dv| <= 32768; reverse 0 / 1.  The u8 arguments are ignored.
 * One launch covers all T windows.  T == 0 returns 0 and launches nothing. */
int augops_resample_u8(const uint8_t *src, long row_pitch, long frame_pitch, int T, int h, int w, int flip, int swap_rb,
                       const int32_t *xmin_x, const int32_t *cnt_x, const int32_t *kk_x, int ksize_x,
                       const int32_t *xmin_y, const int32_t *cnt_y, const int32_t *kk_y, int ksize_y,
                       int oh, int ow, int stage,
                       uint8_t *out_u8, long out_row_pitch, long out_frame_pitch,
                       float *out_f32, int Hp, int Wp, const float *lut, const int32_t *hsv_div, int use_hsv,
                       int dh, int ds, int dv, int reverse, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AUGMENT_OPS_HIP_H */

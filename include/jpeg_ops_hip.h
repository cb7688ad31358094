/* jpeg_ops_hip.h -- C ABI of libjpeg_ops_hip.so: a baseline JPEG stream to interleaved uint8 pixels in two stages.
 *
 *   host    jpegops_parse_header / jpegops_entropy_decode[_batch]: marker parsing and Huffman decoding (plain C++,
 *           csrc/jpeg_entropy_core.h; no HIP call, no device needed) into int16 coefficient blocks and uint16
 *           quantisation tables, typically written straight into pinned memory;
 *   device  jpegops_decode_pixels_u8: dequantisation + 8x8 IDCT (one launch) and chroma upsampling + YCbCr -> RGB +
 *           interleaving (a second launch) on gfx950.
 *
 * The arithmetic ("JPEG decode") is libjpeg-turbo's default decode path in 32-bit integers: the accurate
 * LL&M IDCT (13 constant bits, 2 pass-1 bits, columns first, descale 11 then 18, + 128, clamp to 0..255), triangle
 * ("fancy") upsampling over the true chroma plane with edge replication (plain replication when the chroma plane is
 * at most 2 samples wide), and the 16-bit fixed-point colour tables.  memotr_amd/data/jpeg.py states the same in
 * numpy; the two agree to the bit, and with Pillow on every stream whose dequantised coefficients stay in 16 bits.
 *
 * What the host stage accepts and the error codes it returns for everything else: csrc/jpeg_entropy_core.h.  Codes
 * >= JPEGOPS_UNSUPPORTED name valid streams of a kind this decoder does not read; codes below it, corrupt data or bad
 * arguments.  Nothing is kept between calls except the text of the calling thread's last error.
 */
#ifndef JPEG_OPS_HIP_H
#define JPEG_OPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPEGOPS_ABI_VERSION 1
#define JPEGOPS_UNSUPPORTED 16
#define JPEGOPS_ERR_LEN 256
#define JPEGOPS_MAX_THREADS 16
#define JPEGOPS_QT_WORDS 192          /* uint16[3][64] per frame */
#define JPEGOPS_TILE_X 64             /* output pixels per workgroup of the colour launch: 64 columns x 16 rows */
#define JPEGOPS_TILE_Y 16

/* Component c has blocks_h[c] x blocks_w[c] blocks (whole MCUs) of 64 int16 in natural order, row-major, starting at
 * element coef_offset[c] of the frame's coefficient array of coef_count elements.  One-component streams have
 * h = v = 1.  Unused component slots are 0. */
typedef struct jpegops_info {
    int32_t width, height, ncomp, hmax, vmax, restart_interval, mcus_x, mcus_y;
    int32_t h[3], v[3], blocks_w[3], blocks_h[3];
    int64_t coef_offset[3];
    int64_t coef_count;
} jpegops_info;

int jpegops_abi_version(void);
const char *jpegops_last_error(void);

/* Sizes only: reads the marker segments up to the scan, no entropy-coded data. */
int jpegops_parse_header(const uint8_t *bytes, size_t n, jpegops_info *info);

/* coef_out: coef_bytes >= 2 * coef_count bytes, every block is written whole; qt_out: JPEGOPS_QT_WORDS uint16. */
int jpegops_entropy_decode(const uint8_t *bytes, size_t n, jpegops_info *info, int16_t *coef_out, size_t coef_bytes,
                           uint16_t *qt_out);

/* n_frames streams on min(n_threads, n_frames, JPEGOPS_MAX_THREADS) threads.  status[i] is frame i's code and
 * errors + i * JPEGOPS_ERR_LEN its message (errors may be NULL).  Returns the number of frames that failed, or -1
 * for a bad argument of the call itself. */
int jpegops_entropy_decode_batch(const uint8_t *const *streams, const size_t *sizes, int n_frames, jpegops_info *infos,
                                 int16_t *const *coef_outs, const size_t *coef_bytes, uint16_t *const *qt_outs,
                                 int *status, char *errors, int n_threads);

/* Bytes of device workspace one frame of this geometry needs (the uint8 planes between the two launches). */
int64_t jpegops_planes_bytes(const jpegops_info *info);

/* The device stage for B frames of one geometry, on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation.  Frame b reads coefficients at coef_dev + b * coef_pitch and tables at qt_dev + b * qt_pitch
 * (pitches in elements; both pointers 16-byte aligned, both pitches multiples of 8), uses planes + b *
 * jpegops_planes_bytes() as workspace (planes 16-byte aligned, planes_bytes >= B * jpegops_planes_bytes()) and writes
 * pixel (y, x) channel c at out[b * frame_pitch + y * row_pitch + 3 * x + c]: R, G, B, or B, G, R with swap_rb.
 * Only those bytes are written: nothing between 3 * width and row_pitch.  B == 0 launches nothing. */
int jpegops_decode_pixels_u8(const int16_t *coef_dev, int64_t coef_pitch, const uint16_t *qt_dev, int64_t qt_pitch,
                             const jpegops_info *info, uint8_t *planes, int64_t planes_bytes, uint8_t *out,
                             int64_t row_pitch, int64_t frame_pitch, int B, int swap_rb, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* JPEG_OPS_HIP_H */

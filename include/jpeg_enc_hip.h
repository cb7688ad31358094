/* jpeg_enc_hip.h -- C ABI of libjpeg_enc_hip.so: interleaved uint8 pixels to a baseline JPEG stream in two stages,
 * the mirror image of jpeg_ops_hip.h.
 *
 *   device  jpegenc_forward_u8: RGB -> YCbCr with edge replication and 2 x 2 chroma averaging (one launch), then the
 *           8x8 forward DCT and quantisation (a second launch) on gfx950, into int16 coefficient blocks;
 *   host    jpegenc_huffman_encode[_batch]: marker segments and the Huffman-coded scan (plain C++,
 *           csrc/jpeg_encode_core.h; no HIP call, no device needed).
 *
 * Scope: 8-bit, three components, 4:4:4 or 4:2:0, quality 1 .. 100, the Annex K tables, no restart markers.  The
 * arithmetic is libjpeg-turbo's default compress path in 32-bit integers; the bytes equal the file
 * Pillow's Image.save(..., "JPEG", quality=q, subsampling=0 | 2) writes.  memotr_amd/data/jpeg_write.py states the
 * same in numpy.  Nothing is kept between calls except the text of the calling thread's last error.
 */
#ifndef JPEG_ENC_HIP_H
#define JPEG_ENC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPEGENC_ABI_VERSION 1
#define JPEGENC_ERR_LEN 256
#define JPEGENC_MAX_THREADS 16
#define JPEGENC_QT_WORDS 192          /* uint16[3][64] per frame: luma, chroma, chroma; natural order */
#define JPEGENC_TILE_X 64             /* luma pixels per workgroup of the colour launch: 64 columns x 16 rows */
#define JPEGENC_TILE_Y 16

/* The block geometry of a frame: the layout of jpegops_info (jpeg_ops_hip.h).  Component c has blocks_h[c] x
 * blocks_w[c] blocks (whole MCUs) of 64 int16 in natural order, row-major, starting at element coef_offset[c] of the
 * frame's coefficient array of coef_count elements. */
typedef struct jpegenc_info {
    int32_t width, height, ncomp, hmax, vmax, restart_interval, mcus_x, mcus_y;
    int32_t h[3], v[3], blocks_w[3], blocks_h[3];
    int64_t coef_offset[3];
    int64_t coef_count;
} jpegenc_info;

int jpegenc_abi_version(void);
const char *jpegenc_last_error(void);

/* The geometry of a width x height frame; hmax = 1: 4:4:4, hmax = 2: 4:2:0. */
int jpegenc_geometry(int width, int height, int hmax, jpegenc_info *info);

/* The Annex K tables scaled libjpeg's way for quality 1 .. 100 into qt_out[JPEGENC_QT_WORDS]. */
int jpegenc_quant_tables(int quality, uint16_t *qt_out);

/* The host stage.  Returns the stream's size in bytes, which is the size needed when it is larger than cap: then
 * only out[0 .. cap) was written and the stream is not complete (out may be NULL with cap 0 to ask for the size).
 * Negative: -1 bad argument or geometry, -2 a table entry outside 1 .. 255, -3 a coefficient that baseline coding
 * cannot express. */
int64_t jpegenc_huffman_encode(const int16_t *coef, const uint16_t *qt, const jpegenc_info *info, uint8_t *out,
                               size_t cap);

/* n_frames frames of one geometry on min(n_threads, n_frames, JPEGENC_MAX_THREADS) threads; sizes[i] is what
 * jpegenc_huffman_encode returns for frame i.  Returns the number of frames with sizes[i] < 0 or > caps[i], or -1 for
 * a bad argument of the call itself. */
int jpegenc_huffman_encode_batch(const int16_t *const *coefs, const uint16_t *const *qts, const jpegenc_info *info,
                                 int n_frames, uint8_t *const *outs, const size_t *caps, int64_t *sizes,
                                 int n_threads);

/* Bytes of device workspace one frame of this geometry needs (the uint8 planes between the two launches). */
int64_t jpegenc_planes_bytes(const jpegenc_info *info);

/* The device stage for B frames of one geometry, on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation.  Frame b reads pixel (y, x) channel c at frame[b * frame_pitch + y * row_pitch + 3 * x + c] (R, G,
 * B, or B, G, R with swap_rb), uses planes + b * jpegenc_planes_bytes() as workspace (16-byte aligned) and writes its
 * coef_count coefficients, dummy blocks filled, at coef_dev + b * coef_pitch (elements; pointer 16-byte aligned,
 * pitch a multiple of 8).  qt: HOST pointer to JPEGENC_QT_WORDS uint16, entries 1 .. 255, passed to the kernel by
 * value.  B == 0 launches nothing. */
int jpegenc_forward_u8(const uint8_t *frame, int64_t row_pitch, int64_t frame_pitch, const jpegenc_info *info,
                       const uint16_t *qt, uint8_t *planes, int64_t planes_bytes, int16_t *coef_dev,
                       int64_t coef_pitch, int B, int swap_rb, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* JPEG_ENC_HIP_H */

/* track_draw_hip.h -- C ABI of libtrack_draw_hip.so: the track overlay (boxes, translucent fill, id labels) drawn
 * into an interleaved uint8 frame on gfx950, one launch, all integer (the numpy statement that is the
 * definition: memotr_amd/render.py draw_tracks_host, which also builds the table).
 *
 * The table: n rows of TRACKDRAW_ROW_WORDS int32 on the device, drawn in table order.
 *   0 .. 3   x1, y1, x2, y2   the box, inclusive corners, any values (clipped to the frame; x2 < x1, y2 < y1 or a
 *                             box wholly off the frame: the row draws nothing)
 *   4        box colour, byte 0 -> channel 0, byte 1 -> channel 1, byte 2 -> channel 2 of the frame
 *   5 .. 8   tx1, ty1, tx2, ty2   the label tab, inclusive corners
 *   9        text colour, packed as word 4
 *   10       number of glyphs, 0 .. 10
 *   11, 12   glyph indices 0 .. 9, four bits each: glyphs 0 .. 7 in word 11 from bit 0, glyphs 8 and 9 in word 12
 *   13 .. 15 0
 * Within a row: fill (pixels of the box shrunk by `thickness`, blended (c * a + p * (255 - a) + 127) / 255 where
 * fill_alpha a > 0), outline (pixels of the box not in the shrunk box, opaque), tab (opaque box colour), text (glyph
 * k's 5 x 7 cells, each font_scale pixels square, at tx1 + 1 + 6 * font_scale * k, ty1 + 1).  A pixel takes the last
 * primitive that covers it.  Nothing outside the boxes and tabs is written in place; out of place those bytes are
 * copies, and only the 3 * width bytes of a row are written.
 */
#ifndef TRACK_DRAW_HIP_H
#define TRACK_DRAW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRACKDRAW_ABI_VERSION 1
#define TRACKDRAW_ERR_LEN 256
#define TRACKDRAW_ROW_WORDS 16
#define TRACKDRAW_MAX_GLYPHS 10
#define TRACKDRAW_TILE_X 64           /* pixels per workgroup: 64 columns x 16 rows, 4 pixels per lane */
#define TRACKDRAW_TILE_Y 16
#define TRACKDRAW_CHUNK 64            /* table rows culled against a tile at a time */

int trackdraw_abi_version(void);
const char *trackdraw_last_error(void);

/* The 10 digit glyphs: 7 rows each, bit 4 the leftmost of 5 columns.  out: 70 bytes. */
void trackdraw_font(uint8_t *out);

/* Pixel (y, x) channel c is in[y * in_pitch + 3 * x + c] and out[y * out_pitch + 3 * x + c]; out == in draws in place
 * (then in_pitch == out_pitch), otherwise the two must not overlap.  table: device pointer, 4-byte aligned.
 * thickness >= 1, font_scale >= 1, fill_alpha 0 .. 255.  On `stream` (hipStream_t as void*), no allocation, no
 * synchronisation; n == 0 launches nothing in place and a copy kernel out of place. */
int trackdraw_draw_u8(const uint8_t *in, int64_t in_pitch, uint8_t *out, int64_t out_pitch, int width, int height,
                      const int32_t *table, int n, int thickness, int font_scale, int fill_alpha, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* TRACK_DRAW_HIP_H */

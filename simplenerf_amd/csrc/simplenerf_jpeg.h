/*
 * simplenerf_jpeg.h -- the JPEG frame encoder of the simplenerf_hip library: 8-bit frames that are already on the device leave it as
 * the entropy-coded segment of a baseline JPEG scan (the frames of a Motion-JPEG video).  Declared beside include/simplenerf_hip.h
 * like simplenerf_png.h (the prototypes of the pinned header groups do not change).  Same conventions: status codes,
 * snerf_last_error, device pointers, enqueue-only on `stream`, no allocation, no synchronisation, every check before the first
 * launch.  ABI version 10 is unchanged -- a caller checks that the symbol exists.
 */
#ifndef SIMPLENERF_JPEG_H
#define SIMPLENERF_JPEG_H

#include <stddef.h>

#include "simplenerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_JPEG_BLOCK_BYTES 208     /* an 8 x 8 block codes to at most 1660 bits (below) */

/* snerf_jpeg_scan: `images` frames of (height, width) pixels of `channels` (1: grey, 3: RGB) bytes each -> per frame the
 * ENTROPY-CODED SEGMENT of ONE baseline sequential (SOF0) Huffman scan: every byte between the SOS header and the EOI marker, with
 * the RSTn markers inside it.  The markers around it (SOI, APP0, DQT, SOF0, DHT, DRI, SOS, EOI) depend on (height, width, channels,
 * quality) alone and are the caller's.
 *   pixels      device (images, height, width[, 3]) bytes, frames back to back
 *   quality     1..100
 *   scans       device (images, bound) bytes, bound = snerf_jpeg_scan_bound_bytes(height, width, channels): frame i's segment starts
 *               at scans + i * bound; bytes past its length are not written
 *   scan_bytes  device (images) long long: the length of each segment, <= bound
 *   workspace   device scratch of at least snerf_jpeg_scan_workspace_bytes(...), 16-byte aligned; no initial state, calls
 *               enqueued on ONE stream may share it
 * Three launches: transform (a workgroup per 8 colour or 32 grey MCUs), emit (a workgroup per MCU row), pack (a workgroup per MCU
 * row).  Every operation below is on integers; x >> n is the arithmetic shift (floor(x / 2^n)), a / b truncates.
 *
 * FIXED BY THE STANDARD (ITU-T T.81)
 * Tables.  Quantisation: the luminance and chrominance tables of Annex K.1, each entry t scaled by the libjpeg rule:
 * s = quality < 50 ? 5000 / quality : 200 - 2 * quality;  q = clamp((t * s + 50) / 100, 1, 255).  Huffman: the four tables of Annex
 * K.3 (DC and AC, luminance and chrominance), canonical codes by Annex C.  Coefficients in the zig-zag order of Figure 5.
 * Layout.  channels == 1: one component (id 1, 1x1 sampling, quantisation table 0, Huffman tables 0/0), MCU = one 8 x 8 block.
 * channels == 3: Y Cb Cr (ids 1 2 3; Y 2x2 sampling, table 0, Huffman 0/0; Cb, Cr 1x1, table 1, Huffman 1/1), MCU = 16 x 16 pixels,
 * its blocks in the order Y00 Y01 Y10 Y11 Cb Cr (Yrc: row r, column c of the 2 x 2 luminance blocks).  MCUs left to right, top to
 * bottom; mcus_per_row = ceil(width / m), mcu_rows = ceil(height / m), m = 8 or 16.
 * Restart interval.  ONE MCU ROW: the DRI segment says mcus_per_row.  The DC predictor of every component is 0 at the start of
 * each interval.  Each interval's bits are padded to a byte with 1-bits; every interval but the frame's last is followed by
 * FF D0+(r mod 8), r = 0, 1, ... its MCU row.  Inside an interval (padding included) a byte FF is followed by a byte 00.
 * Coefficient coding.  DC: diff = DC - predictor, category = bits of |diff| (0..11), the Huffman code of the category, then the
 * low `category` bits of diff (diff >= 0) or of diff - 1 (diff < 0).  AC, for k = 1..63: a non-zero level after `run` zeros: while
 * run >= 16, ZRL (symbol F0) and run -= 16; then the code of symbol (run << 4 | size), size = bits of |level| (1..10), then `size`
 * bits as for DC.  A block whose last coefficients are zero ends with EOB (symbol 00); a block whose 63rd coefficient is not zero
 * has no EOB.  Bits are written most significant first.
 *
 * THIS ENCODER'S OWN CHOICES
 * Edges.  A frame is padded to whole MCUs by repeating its last column and its last row: pixel (y, x) of the padded frame is pixel
 * (min(y, height - 1), min(x, width - 1)).  Padding comes before colour conversion and subsampling.
 * Colour (channels == 3), per pixel, 16-bit fixed point of the JFIF full-range matrix:
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16          8421375 = 128 * 65536 + 32767
 *   Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16
 * All three are in 0..255 for every input; nothing is clamped.
 * Chroma.  Each Cb / Cr sample is (a + b + c + d + 2) >> 2 over the 2 x 2 cell of per-pixel Cb / Cr values.
 * DCT.  Of s = sample - 128, separable, rows then columns, each 1-D pass a plain product with the 8 x 8 integer matrix
 *   D[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)),  a(0) = sqrt(1/8), a(u > 0) = 1/2,
 * whose entries are D[0][x] = 2896 and, for u > 0, +-c[k] with c[1..7] = 4017 3784 3406 2896 2276 1567 799 (= round(4096 cos(k pi /
 * 16))), k and the sign those of cos((2 x + 1) u pi / 16) folded into the first quadrant (the matrix is spelled out in
 * csrc/jpeg_coder.h).  No butterfly factorisation: 64 multiply-adds per pass and row.
 *   rows:     t[y][u]  = (sum_x D[u][x] s[y][x] + 1024) >> 11          (4 x the 1-D transform)
 *   columns:  F8[v][u] = (sum_y D[v][y] t[y][u] + 2048) >> 12          (8 x the orthonormal 2-D DCT, the FDCT of T.81 A.3.3)
 * Every intermediate fits 32 bits.
 * Quantisation.  level = sign(F8) * ((|F8| + 4 q) / (8 q)): division by 8 q rounded half away from zero.  Levels are limited to
 * -1023..1023 (AC) and -1024..1023 (DC); 8-bit samples never reach the limits.
 *
 * Bound.  The longest DC code has 11 bits and carries 11 more; the longest AC code has 16 bits and carries 10: a block is at most
 * 22 + 63 * 26 = 1660 bits <= SNERF_JPEG_BLOCK_BYTES bytes.  Stuffing at most doubles an interval's bytes (its padding byte
 * included), and its marker adds 2.  With blocks_per_row = mcus_per_row * (channels == 3 ? 6 : 1):
 *   snerf_jpeg_scan_bound_bytes = mcu_rows * (2 * SNERF_JPEG_BLOCK_BYTES * blocks_per_row + 2);  no input produces more.
 *
 * Determinism.  Integer arithmetic only; the LDS atomics (OR-ing codes into the bit buffer) are order-free.  Two calls give the
 * same bytes, and frame i's segment does not depend on `images` or on the other frames.
 *
 * Errors.  channels not 1 or 3, height or width outside 1..65535, quality outside 1..100, images < 0, or images > 0 with a NULL
 * pointer, a workspace that is not 16-byte aligned or a scan_bytes that is not 8-byte aligned: SNERF_E_INVALID.  images x
 * mcu_rows x chunks per row (the transform's workgroups) >= 2^31: SNERF_E_UNSUPPORTED.  images == 0 enqueues nothing and returns
 * SNERF_OK.  The two queries return 0 for arguments the call rejects. */
size_t snerf_jpeg_scan_bound_bytes(int height, int width, int channels); /* per frame */
size_t snerf_jpeg_scan_workspace_bytes(int images, int height, int width, int channels);
int snerf_jpeg_scan(const unsigned char* pixels, int images, int height, int width, int channels, int quality,
                    unsigned char* scans, long long* scan_bytes, void* workspace, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_JPEG_H */

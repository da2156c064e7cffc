/*
 * simplenerf_png.h -- the PNG frame encoder of the simplenerf_hip library: 8-bit frames that are already on the device leave it as
 * the payload of their file's IDAT chunk.  Declared beside include/simplenerf_hip.h like simplenerf_maps.h (the prototypes of the
 * pinned header groups do not change).  Same conventions: status codes, snerf_last_error, device pointers, enqueue-only on
 * `stream`, no allocation, no synchronisation, every check before the first launch.  ABI version 10 is unchanged -- a caller checks
 * that the symbol exists.
 */
#ifndef SIMPLENERF_PNG_H
#define SIMPLENERF_PNG_H

#include <stddef.h>

#include "simplenerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_PNG_FILTER_ADAPTIVE -1   /* filter_mode: each row takes the type the rule below picks; 0..4: that type on every row */
#define SNERF_PNG_STRIP_BYTES 32768    /* filtered bytes coded by one workgroup as one deflate block */

/* snerf_png_deflate: `images` frames of (height, width) pixels of `channels` (1: grey, 3: RGB) bytes each -> per frame one complete
 * ZLIB STREAM, the payload of ONE IDAT chunk: the 2-byte header 78 9C, deflate blocks, the big-endian Adler-32 of the filtered
 * bytes.  Inflating it gives exactly raw = height * (1 + width * channels) bytes: per row the filter type, then the filtered row;
 * un-filtered by the PNG rules they are the pixels.  The container (signature, IHDR, the IDAT length and CRC-32, IEND) is the caller's.
 *   pixels        device (images, height, width[, 3]) bytes, frames back to back
 *   streams       device (images, bound) bytes, bound = snerf_png_deflate_bound_bytes(height, width, channels): frame i's stream
 *                 starts at streams + i * bound; bytes past its length are not written
 *   stream_bytes  device (images) long long: the length of each stream, <= bound
 *   workspace     device scratch of at least snerf_png_deflate_workspace_bytes(...), 16-byte aligned; no initial state, calls
 *                 enqueued on ONE stream may share it
 * Four launches: filter (a workgroup per row), code (a workgroup per strip), scan (a workgroup per frame), pack (a workgroup per
 * strip).
 *
 * Filtering.  One pass; rows are independent: a row reads the RAW row above it, never filtered data; the first row treats the row
 * above as zeros; bpp = channels.  filter_mode = -1: a row takes the type t in 0..4 (None, Sub, Up, Average, Paeth) that minimises
 * sum(min(v, 256 - v)) over its width * channels filtered bytes v (the type byte is not counted); a tie goes to the lowest type.
 * The choice depends on the row and the row above alone, so it is the same on every run and whatever else is in the call.
 *
 * Strips.  Each frame's filtered stream is cut into strips of SNERF_PNG_STRIP_BYTES consecutive bytes (the last is shorter; rows
 * do not matter).  Each strip is coded on its own: literals, and matches at distance 1 only, of length 3..258 -- a byte repeated,
 * zlib's Z_RLE.  A run of r equal bytes inside a strip is one literal, then matches of 258 while more than 258 bytes are left, then
 * one match of what is left, or one or two literals when that is less than 3.  No match reaches back across the start of its strip.
 * A strip is ONE dynamic-Huffman block (BTYPE=10): its own literal/length code of lengths <= 15, complete and not over-subscribed,
 * described through a code-length code of lengths <= 7 (complete too).  The lengths are those of a Huffman code of the strip's
 * symbol counts; while that code is deeper than the limit every count c becomes (c + 1) / 2 and the code is built again.  A strip
 * with no match declares one distance code of length 0, a strip with matches one distance code of one bit.  A strip whose coded
 * form would not be smaller than its stored form is written as a stored block (BTYPE=00).
 *
 * Stitching.  Every strip but the last ends on a byte boundary: where its block does not, an empty stored block (three zero
 * header bits, zero padding, 00 00 FF FF) follows it.  The last strip carries BFINAL.  Strips are packed to their byte offsets by
 * a scan over the strip sizes; the Adler-32 is combined in strip order from per-strip (s1, s2) pairs.
 *
 * Bound.  snerf_png_deflate_bound_bytes = raw + 5 per started strip + 6 (<= raw + 10 per started strip + 6); no input produces more.
 *
 * Determinism.  Integer arithmetic only; the LDS atomics (histogram adds, OR-ing codes into the bit buffer) are order-free.  Two
 * calls give the same bytes, and frame i's stream does not depend on `images` or on the other frames.
 *
 * Errors.  channels not 1 or 3, height or width < 1, filter_mode outside -1..4, raw >= 2^31, images < 0, or images > 0 with a NULL
 * pointer or a workspace that is not 16-byte aligned: SNERF_E_INVALID.  images x height or images x strips >= 2^31:
 * SNERF_E_UNSUPPORTED.  images == 0 enqueues nothing and returns SNERF_OK.  The two queries return 0 for arguments the call rejects. */
size_t snerf_png_deflate_bound_bytes(int height, int width, int channels); /* per frame */
size_t snerf_png_deflate_workspace_bytes(int images, int height, int width, int channels);
int snerf_png_deflate(const unsigned char* pixels, int images, int height, int width, int channels, int filter_mode,
                      unsigned char* streams, long long* stream_bytes, void* workspace, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_PNG_H */

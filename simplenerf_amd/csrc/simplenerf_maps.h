/*
 * simplenerf_maps.h -- an entry point of the simplenerf_hip library that is declared beside include/simplenerf_hip.h instead of
 * in it: the prototypes of the two headers under include/ are a pinned set.  Same conventions (status codes, snerf_last_error,
 * device pointers, `stream`); ABI version 10 is unchanged -- no existing struct or signature changed, a caller checks that the
 * symbol exists.
 */
#ifndef SIMPLENERF_MAPS_H
#define SIMPLENERF_MAPS_H

#include "simplenerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The 8-bit previews the reference's trainer writes beside its float maps (src/Trainer01.py: save_image :384-387,
 * save_numpy_array :397-409), for all maps of a frame in one call of two launches.
 *   maps       device (num_maps, n) fp32, map k at maps + k * n (4-byte aligned; a map that starts on a 16-byte boundary, or
 *              reaches one within its first three values, is read 16 bytes at a time from there)
 *   modes      device (num_maps) int: 0 = rint(x * 255) (a colour image is 3 n values of mode 0, in any split);
 *              1 = rint(x / max(x) * 255), max over the map's n values
 *   out        device (num_maps, n) bytes;  status  device (num_maps) int, written for every map
 *   workspace  device scratch of at least the query below; no initial state, calls enqueued on ONE stream may share it
 * Arithmetic is numpy's float32 arithmetic, operation for operation: the map's maximum first (exact in any order), then one
 * IEEE fp32 division, one fp32 multiplication by 255 and round-half-to-even -- no reciprocal, no contraction.
 * Where numpy's own uint8 cast is undefined the rule is this library's: the rounded value saturates to 0..255 (-inf and every
 * negative -> 0, +inf -> 255, NaN -> 0); a mode-1 map whose maximum is not a positive finite number (0, negative, NaN -- numpy's
 * maximum propagates NaN -- or +inf) gives n zeros and status 1, a mode other than 0 or 1 gives n zeros and status 2, every other
 * map status 0; a map never affects its neighbours.  num_maps == 0 or n == 0 enqueues nothing and returns SNERF_OK;
 * num_maps > 65535, a negative count and a NULL pointer are SNERF_E_INVALID.  No atomics; only enqueues on `stream`. */
long long snerf_maps_to_u8_workspace_bytes(int num_maps);
int snerf_maps_to_u8(const float* maps, const int* modes, int num_maps, long long n, unsigned char* out, int* status,
                     void* workspace, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_MAPS_H */

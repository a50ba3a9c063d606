/*
 * nlzm_hip_elem.h -- C ABI of the choice of a typed range's element size, made on the device from plane statistics.  A header of its own beside
 * nlzm_hip.h, which it includes: conventions, error codes, nlzm_hip_last_error() and nlzm_hip_get_counter() are that header's, and the functions are
 * exported by the same library.
 *
 * nlzm_hip_compress_ranges_typed* (nlzm_hip.h) takes an element size per range as given.  Here the sizes are chosen: one bandwidth-bound pass over the
 * ranges' bytes counts them, and a rule in integers picks 1, 2, 4 or 8.  The rule (nlzm_amd/csrc/nlzm_elem.h and nlzm_elem_plan.h; tests/elem_model.py
 * restates it): for a range x of n bytes, M = n div 8, H[c][v] is the number of i < 8 M with i mod 8 = c and x[i] = v -- i counted from the range's own
 * first byte; no address and no alignment enters, and the n mod 8 bytes behind are in no histogram.  The planes of element size e are
 * P(e, j)[v] = the sum over c = j (mod e) of H[c][v], j < e.  L(n) is the binary logarithm in 2^-16 bits: L(0) = L(1) = 0; for n >= 2,
 * k = floor(log2 n), x = floor(n 2^31 / 2^k), r = k 2^16, and for i = 15 .. 0: x = floor(x^2 / 2^31); if x >= 2^32: x = floor(x / 2), r += 2^i;
 * L(n) = r.  cost(h) = N L(N) - sum h[v] L(h[v]) + floor(K L(N) / 2) modulo 2^64 for a histogram of total N with K non-zero bins, and C_e is the sum
 * of cost(P(e, j)) over j < e.  The choice for a range of n bytes: 1 when n < 4096; otherwise b, the e of smallest C_e (ties to the smaller e),
 * unless b != 1 and C_b + floor(C_1 / 32) > C_1: then 1.
 *
 * k: 1 .. 65536; off / len: host arrays of k entries; the ranges may be empty, overlap and repeat.  All NLZM_HIP_E_ARG, the text naming the range,
 * checked before any launch, with or without a device: a range that runs over its buffer, a range of 2^40 bytes or more (N L(N) has to fit 64 bits).
 * Reads stay inside the ranges: no padding, no alignment is asked for.  Without a device the calls end in NLZM_HIP_E_NODEVICE after these checks.
 * Device memory of a call beyond its input, freed before it returns: 40 bytes a range of table at most, 32 bytes a range of costs, and 16 KiB for every range
 * of more than nlzm_hip_get_counter("elem_segment_bytes") bytes (for every range where hist is asked for); NLZM_HIP_E_NOMEM when there is no room,
 * and nothing is left open.
 * Counters of the last call: "elem_us" (device time of its launches), "elem_bytes" (the bytes of its ranges), "elem_segment_bytes" (needs no device).
 */
#ifndef NLZM_HIP_ELEM_H
#define NLZM_HIP_ELEM_H

#include "nlzm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (C_1, C_2, C_4, C_8) of every range: cost has 4 k entries.  hist may be NULL; else k * 2048 entries, H[c][v] of range i at hist[(i * 8 + c) * 256 + v]. */
int nlzm_hip_plane_costs_dev(const void *d_buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint64_t *cost, uint64_t *hist);
int nlzm_hip_plane_costs(const uint8_t *buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint64_t *cost, uint64_t *hist);   /* uploads first */
/* the choice for one range; pure, needs no device, cannot fail */
uint32_t nlzm_hip_choose_elem(const uint64_t *cost4, uint64_t len);
/* costs and choice in one call: elem has k entries, each 1, 2, 4 or 8 */
int nlzm_hip_choose_elems_dev(const void *d_buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem);
int nlzm_hip_choose_elems(const uint8_t *buf, uint64_t buf_len, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem);
/* nlzm_hip_compress_ranges_typed* with the element sizes chosen first and handed back in elem_out (k entries, must not be NULL): stream i is the
 * typed call's for elem_out[i], nlzm_hip_decompress_blocks_typed* reads the result with elem_out, and arguments, errors, bound, counters and option
 * "dedup_ranges" are the typed call's */
int nlzm_hip_compress_ranges_auto_dev(const void *d_src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem_out,
                                      uint32_t hist_bits_req, void *d_dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);
int nlzm_hip_compress_ranges_auto(const uint8_t *src, uint64_t n, uint32_t k, const uint64_t *off, const uint64_t *len, uint8_t *elem_out,
                                  uint32_t hist_bits_req, uint8_t *dst, uint64_t dst_cap, uint64_t *block_len, uint64_t *dst_len);

#ifdef __cplusplus
}
#endif

#endif

/* sdhip_ingest_test.h -- test hook of k_many_ingest (csrc/ingest.hip), the fill kernel of sd_diarize_many_audio*.  Not part of the drop-in boundary
 * (sdhip.h) and kept apart from sdhip_test.h, whose list of entries tests/test_abi.py pins name by name. */
#ifndef SDHIP_INGEST_TEST_H
#define SDHIP_INGEST_TEST_H
#include "sdhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ONE k_many_ingest launch, through the function the product calls for it (launch_many_ingest), on rows the test chooses.
 * rows [R][8] = (encoding, channels, channel, sample_rate, n, src_off, base, len): n frames whose first element lies src_off BYTES into src (a multiple
 * of the element size; -1 with n == 0: no source), decoded by the rule of sdhip.h into dst[base, base + len16) with zeros up to dst[base + len).
 * Every row's source is laid out on the device on its own with 256 guard elements behind the last element the rule reads: NaN for floats, 0x7fff for
 * int16, the code of the law's largest magnitude for G.711.  dst has dst_len floats of `canary` and 256 more behind them; all dst_len + 256 come back in
 * dst_out.  SD_ERR_ARG before any launch: a bad descriptor or rate pair, len16 > len, a row that leaves dst or src, two rows that share a destination. */
int sd_test_many_ingest(sd_ctx*, const int64_t* rows /*[R][8]*/, int64_t R, const void* src, int64_t src_bytes, int64_t dst_len, float canary, float* dst_out /*[dst_len + 256]*/);

#ifdef __cplusplus
}
#endif
#endif

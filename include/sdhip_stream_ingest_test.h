/* sdhip_stream_ingest_test.h -- test hook of k_group_ingest (csrc/stream_ingest.hip), the decode kernel of sd_stream_push_audio* and
 * sd_stream_push_many_audio*.  Not part of the drop-in boundary (sdhip.h) and kept apart from sdhip_test.h, whose list of entries tests/test_abi.py pins
 * name by name. */
#ifndef SDHIP_STREAM_INGEST_TEST_H
#define SDHIP_STREAM_INGEST_TEST_H
#include "sdhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ONE k_group_ingest launch, through the function the product calls for it (launch_group_ingest, pad = SD_TAIL_PAD = 512), on rows the test chooses.
 * rows [R][7] = (encoding, channels, channel, n, src_off, dst_off, room): n frames whose first element lies src_off BYTES into src (a multiple of the
 * element size), decoded by steps 1 and 2 of the rule of sdhip.h into dst[dst_off, dst_off + n), 512 zeros behind, nothing at or behind
 * dst[dst_off + room].  Rows with equal (src_off, n, encoding, channels) share a source: every distinct source is laid out on the device on its own, at
 * src_off mod 16 bytes behind a 16-byte boundary (so the test chooses which rows can take the wide loads), with 256 guard elements behind the last
 * element the rule reads for the rows that share it: NaN for floats, 0x7fff for int16, the code of the law's largest magnitude for G.711.  dst has
 * dst_len floats of `canary` and 256 more behind them; all dst_len + 256 come back in dst_out.  SD_ERR_ARG before any launch: a bad format, a row
 * that leaves src or dst, two rows that share a destination. */
int sd_test_group_ingest(sd_ctx*, const int64_t* rows /*[R][7]*/, int64_t R, const void* src, int64_t src_bytes, int64_t dst_len, float canary, float* dst_out /*[dst_len + 256]*/);

#ifdef __cplusplus
}
#endif
#endif

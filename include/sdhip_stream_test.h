/* sdhip_stream_test.h -- test hook of the streams (csrc/stream.hip).  Not part of the drop-in boundary (sdhip.h) and kept apart from sdhip_test.h,
 * whose list of entries tests/test_abi.py pins name by name. */
#ifndef SDHIP_STREAM_TEST_H
#define SDHIP_STREAM_TEST_H
#include "sdhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The f32 samples a stream holds on the device: those from sample sealed * 8000 on (sd_stream_info), *n of them, the first being sample *first_sample
 * of everything the stream was given at 16 kHz (the origin of a window included).  At most cap samples are expected: cap < *n is SD_ERR_ARG with *n
 * set; h_out == NULL only sets *n and *first_sample. */
int sd_test_stream_tail(sd_stream*, float* h_out, int64_t cap, int64_t* n, int64_t* first_sample);

#ifdef __cplusplus
}
#endif
#endif

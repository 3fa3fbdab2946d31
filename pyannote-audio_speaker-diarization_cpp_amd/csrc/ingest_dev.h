// ingest_dev.h -- the staging load of a recording or of a stream's piece, the one device text of steps 1 (decode) and 2 (channel) of the rule of
// include/sdhip.h ("recordings in their own rate and encoding"): k_many_ingest (ingest.hip) passes it to resample_point (resample_dev.h),
// k_group_ingest (stream_ingest.hip) stores what it returns.  G.711 is ingest_plan.h's text, which the host entries run too.
#pragma once
#include "common.h"
#include "ingest_plan.h"

// The staging load of a recording: frame i -> the float of the rule's steps 1 and 2.
// The mean of the channels is wav_load's loop (wav_file.h): s = +0.0f, s += x_q in channel order, s / (float)channels.  The division must be the
// correctly rounded one, as the host's is: __fdiv_rn is IEEE division under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt (the Makefile
// passes neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt); a reciprocal multiply differs at 3 channels.
struct IngestLoad {
    const void* __restrict__ src; int enc, channels, channel;
    __device__ __forceinline__ float elem(int64_t e) const
    {
        switch (enc) {
        case SD_ENC_S16: return pcm_to_float(((const int16_t*)src)[e]);
        case SD_ENC_F32: return ((const float*)src)[e];
        case SD_ENC_MULAW: return pcm_to_float((int16_t)g711_mulaw(((const uint8_t*)src)[e]));
        default: return pcm_to_float((int16_t)g711_alaw(((const uint8_t*)src)[e]));
        }
    }
    // the same decode of an element that is already in a register, in the low 8 / 16 / 32 bits of v (the wide loads of k_group_ingest)
    __device__ __forceinline__ float of_bits(uint32_t v) const
    {
        switch (enc) {
        case SD_ENC_S16: return pcm_to_float((int16_t)(v & 0xffffu));
        case SD_ENC_F32: return __uint_as_float(v);
        case SD_ENC_MULAW: return pcm_to_float((int16_t)g711_mulaw(v & 0xffu));
        default: return pcm_to_float((int16_t)g711_alaw(v & 0xffu));
        }
    }
    __device__ __forceinline__ float operator()(int64_t i) const
    {
        if (channel >= 0) return elem(i * channels + channel);
        float s = 0.0f;
        for (int q = 0; q < channels; ++q) s += elem(i * channels + q);
        return __fdiv_rn(s, (float)channels);
    }
};

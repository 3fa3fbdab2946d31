// wav_file.h -- the wav reader (a1, wav.h:62-126) and the rule that turns a wav file into the 16 kHz mono samples the pipeline diarizes.
// Plain C++ without a GPU header: the library (api.cpp, pipeline.cpp), the command line and the stand-alone sanitizer program
// (tools/sanitize/wav_file_main.cpp) include the same text.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/sdhip.h"

// bytes of the data chunk that are really in the file.  A wav written to a pipe (ffmpeg, sox) announces 0xFFFFFFFF (or 0) because the
// writer could not seek back; the reference trusts the header (wav.h:92-97) and would "read" two billion samples from a short file.
// Deliberate deviation, input robustness only: what is announced beyond the end of the file is not read, and a size of
// 0xFFFFFFFF means "up to the end of the file"; so does 0, unless what follows the empty data chunk is a well-formed chain of RIFF
// sub-chunks (LIST, id3 ...) -- then the file really has no samples, as the reference reads it.
inline uint32_t data_bytes_present(FILE* fp, uint32_t announced)
{
    const long cur = ftell(fp);
    if (cur < 0 || fseek(fp, 0, SEEK_END) != 0) return announced;
    const long end = ftell(fp);
    (void)fseek(fp, cur, SEEK_SET);
    if (end < cur) return announced;
    const uint64_t remaining = (uint64_t)(end - cur);
    const uint32_t to_end = (uint32_t)(remaining > 0xFFFFFFFEull ? 0xFFFFFFFEull : remaining);
    if (announced == 0xFFFFFFFFu || (uint64_t)announced > remaining) return to_end;
    if (announced == 0 && remaining > 0) {
        // 0 is what some stream writers leave -- but also what a well-formed file with an EMPTY data chunk followed by LIST / id3
        // metadata says (the reference reads 0 samples there).  Stream rule only when what follows is NOT a chain of RIFF sub-chunks
        // that ends exactly at the end of the file.
        long pos = cur;
        bool chain = true;
        while (pos < end) {
            unsigned char t8[8];
            if (end - pos < 8 || fseek(fp, pos, SEEK_SET) != 0 || fread(t8, 1, 8, fp) != 8) { chain = false; break; }
            for (int q = 0; q < 4; ++q) if (t8[q] < 0x20 || t8[q] > 0x7e) chain = false;
            uint32_t sz; memcpy(&sz, t8 + 4, 4);
            if (!chain || (uint64_t)sz > (uint64_t)(end - pos - 8)) { chain = false; break; }
            pos += 8 + (long)sz;
            if (pos < end && (sz & 1) && end - pos >= 1) pos += 1;      // RIFF pad byte
        }
        (void)fseek(fp, cur, SEEK_SET);
        return chain ? 0u : to_end;
    }
    return announced;
}

// The header walk both readers share (wav.h:62-90): the 44-byte canonical header, a longer fmt chunk (75-79), LIST / fact / ...
// sub-chunks in front of the data (85-90).  On success the file is positioned on the first data byte and *dsz holds the bytes of
// data really present.  Returns nullptr (file closed) when the file cannot be opened or ends inside its headers.
inline FILE* wav_open_data(const char* path, uint32_t* sr, uint16_t* ch, uint16_t* bits, uint32_t* dsz)
{
    FILE* fp = fopen(path, "rb");
    if (!fp) return nullptr;                          // reference ignores this (wav.h:60) and crashes later
    unsigned char h[44];
    if (fread(h, 1, 44, fp) != 44) { fclose(fp); return nullptr; }
    uint32_t fmt_size; char tag[4];
    memcpy(&fmt_size, h + 16, 4); memcpy(ch, h + 22, 2); memcpy(sr, h + 24, 4); memcpy(bits, h + 34, 2);
    memcpy(tag, h + 36, 4); memcpy(dsz, h + 40, 4);
    if (fmt_size < 16) { fclose(fp); return nullptr; }
    unsigned char t8[8];
    if (fmt_size > 16) {                               // wav.h:75-79
        fseek(fp, 44 - 8 + (long)fmt_size - 16, SEEK_SET);
        if (fread(t8, 1, 8, fp) != 8) { fclose(fp); return nullptr; }
        memcpy(tag, t8, 4); memcpy(dsz, t8 + 4, 4);
    }
    while (strncmp(tag, "data", 4) != 0) {             // wav.h:85-90 skip LIST/fact chunks
        fseek(fp, (long)*dsz, SEEK_CUR);
        if (fread(t8, 1, 8, fp) != 8) { fclose(fp); return nullptr; }
        memcpy(tag, t8, 4); memcpy(dsz, t8 + 4, 4);
    }
    *dsz = data_bytes_present(fp, *dsz);
    return fp;
}

// sd_read_wav: the 16-bit samples as they are, malloc'd (free)
inline int wav_read_pcm16(const char* path, int16_t** pcm, int64_t* n, int32_t* sample_rate, int32_t* channels)
{
    if (!path || !pcm || !n) return SD_ERR_ARG;
    *pcm = nullptr; *n = 0;
    uint32_t sr, dsz; uint16_t ch, bits;
    FILE* fp = wav_open_data(path, &sr, &ch, &bits, &dsz);
    if (!fp) return SD_ERR_ARG;
    if (bits != 16) { fclose(fp); return SD_ERR_ARG; } // README.md:37: 16 kHz / mono / 16 bit only
    int64_t num = dsz / 2;
    int16_t* buf = (int16_t*)malloc((size_t)(num > 0 ? num : 1) * sizeof(int16_t));
    int64_t got = (int64_t)fread(buf, 2, (size_t)num, fp);
    for (int64_t i = got; i < num; ++i) buf[i] = 0;
    fclose(fp);
    *pcm = buf;
    *n = num / (ch ? ch : 1);                          // wav.h:97 (interleaved data read as mono)
    if (sample_rate) *sample_rate = (int32_t)sr;
    if (channels) *channels = ch;
    return SD_OK;
}

// sd_read_wav_f32: all bit depths the reference reads (wav.h:99-122).  8-bit samples are read as signed char, 32-bit as int, every depth
// is then divided by 32768 (sd.cpp:2950) -- the reference's scaling, kept as is.  malloc'd float samples (free)
inline int wav_read_f32(const char* path, float** wav, int64_t* n, int32_t* sample_rate, int32_t* channels, int32_t* bits_per_sample)
{
    if (!path || !wav || !n) return SD_ERR_ARG;
    *wav = nullptr; *n = 0;
    uint32_t sr, dsz; uint16_t ch, bits;
    FILE* fp = wav_open_data(path, &sr, &ch, &bits, &dsz);
    if (!fp) return SD_ERR_ARG;
    if (bits != 8 && bits != 16 && bits != 32) { fclose(fp); return SD_ERR_ARG; }     // reference: exit(1), wav.h:119-121
    const int bps = bits / 8;
    const int64_t num = dsz / bps;
    std::vector<unsigned char> raw((size_t)(num > 0 ? num * bps : 1));
    const size_t got = fread(raw.data(), 1, (size_t)num * bps, fp);
    fclose(fp);
    if (got < (size_t)num * bps) memset(raw.data() + got, 0, (size_t)num * bps - got);
    float* out = (float*)malloc(sizeof(float) * (size_t)(num > 0 ? num : 1));
    for (int64_t i = 0; i < num; ++i) {
        float v;
        if (bits == 8) v = (float)(signed char)raw[(size_t)i];
        else if (bits == 16) { int16_t s; memcpy(&s, &raw[(size_t)i * 2], 2); v = (float)s; }
        else { int32_t s; memcpy(&s, &raw[(size_t)i * 4], 4); v = (float)s; }
        out[i] = (float)((double)(v * 1.0f) / 32768.0);
    }
    *wav = out;
    *n = num / (ch ? ch : 1);
    if (sample_rate) *sample_rate = (int32_t)sr;
    if (channels) *channels = ch;
    if (bits_per_sample) *bits_per_sample = bits;
    return SD_OK;
}

// sd_read_wav_audio: the file as it is, for sd_diarize_many_audio -- the header walk of wav_open_data, but the format tag (h + 20) is read: tag 1 with 16
// bits (SD_ENC_S16), tag 7 with 8 bits (mu-law), tag 6 with 8 bits (A-law); any channel count >= 1, any rate > 0; the data bytes counted by
// data_bytes_present, whole frames only.  *data = the malloc'd raw bytes (free), *desc filled with data = *data and channel = 0.  Any other file --
// other tags or depths (WAVE_FORMAT_EXTENSIBLE, float, 24-bit, 8-bit PCM), a header that ends early -- is SD_ERR_ARG with nothing allocated.
inline int wav_read_audio(const char* path, sd_audio* desc, void** data)
{
    if (!path || !desc || !data) return SD_ERR_ARG;
    *data = nullptr;
    unsigned char h[22];
    uint16_t tag = 0;
    {
        FILE* f0 = fopen(path, "rb");
        if (!f0) return SD_ERR_ARG;
        const size_t got = fread(h, 1, 22, f0);
        fclose(f0);
        if (got != 22) return SD_ERR_ARG;
        memcpy(&tag, h + 20, 2);
    }
    uint32_t sr, dsz; uint16_t ch, bits;
    FILE* fp = wav_open_data(path, &sr, &ch, &bits, &dsz);
    if (!fp) return SD_ERR_ARG;
    int32_t enc;
    if (tag == 1 && bits == 16) enc = SD_ENC_S16;
    else if (tag == 7 && bits == 8) enc = SD_ENC_MULAW;
    else if (tag == 6 && bits == 8) enc = SD_ENC_ALAW;
    else { fclose(fp); return SD_ERR_ARG; }
    if (ch < 1 || sr == 0 || sr > 0x7fffffffu) { fclose(fp); return SD_ERR_ARG; }
    const int64_t frame = (int64_t)ch * (bits / 8), n = (int64_t)dsz / frame, bytes = n * frame;
    unsigned char* buf = (unsigned char*)malloc((size_t)(bytes > 0 ? bytes : 1));
    if (!buf) { fclose(fp); return SD_ERR_ARG; }
    const size_t got = fread(buf, 1, (size_t)bytes, fp);
    fclose(fp);
    if (got < (size_t)bytes) memset(buf + got, enc == SD_ENC_S16 ? 0 : enc == SD_ENC_MULAW ? 0xff : 0xd5, (size_t)bytes - got);      // (cannot happen: the bytes were counted; silence in each law)
    *data = buf;
    desc->data = buf; desc->n = n; desc->sample_rate = (int32_t)sr; desc->encoding = enc; desc->channels = ch; desc->channel = 0;
    return SD_OK;
}

// ---- the loading rule of sd_diarize_wav / sd_activity_wav / sd_voiceprint_wav and of the command line (flags = SD_WAV_*):
//   the 16-bit reader's int16 samples when the rate is 16 000 (or ASSUME_16K: the reference's behaviour, sd.cpp:2940-2942) and the file is not
//   multi-channel under DOWNMIX -- the common case stays int16 up to the GPU;
//   otherwise the all-depth reader's floats, the channels averaged under DOWNMIX: taken at 16 000 / ASSUME_16K, to be resampled by the caller from
//   `sr` under RESAMPLE, refused without it.
struct WavLoad {
    enum Kind { PCM16, F32, F32_OFF_RATE,             // n samples in pcm / in f32 / in f32 at `sr` Hz: the caller resamples them to 16 kHz
                UNREADABLE, OFF_RATE, NO_SAMPLES };   // refusals: no PCM wav of 8, 16 or 32 bits / not 16 kHz and no flag / RESAMPLE of an empty file
    Kind kind = UNREADABLE;
    int16_t* pcm = nullptr; float* f32 = nullptr;
    int64_t n = 0; int32_t sr = 0;
    std::string msg;                                  // of a refusal; says nothing of the path: the caller puts it where its own lines have it
    WavLoad() = default; WavLoad(const WavLoad&) = delete; WavLoad& operator=(const WavLoad&) = delete;      // owns pcm and f32
    ~WavLoad() { free(pcm); free(f32); }
    bool refused() const { return kind >= UNREADABLE; }
    // a refusal as a line of its own, the path where the whole-path entries have always had it
    std::string refusal(const char* path) const
    {
        return kind == UNREADABLE ? msg + ": " + path : kind == OFF_RATE ? std::string(path) + ": " + msg : std::string(path) + " " + msg;
    }
};

inline void wav_load(const char* path, int flags, WavLoad& w)
{
    int32_t ch = 0;
    if (wav_read_pcm16(path, &w.pcm, &w.n, &w.sr, &ch) == SD_OK) {
        if ((w.sr == 16000 || (flags & SD_WAV_ASSUME_16K)) && !(ch > 1 && (flags & SD_WAV_DOWNMIX))) { w.kind = WavLoad::PCM16; return; }
        free(w.pcm); w.pcm = nullptr;
    }
    if (wav_read_f32(path, &w.f32, &w.n, &w.sr, &ch, nullptr) != SD_OK) { w.kind = WavLoad::UNREADABLE; w.msg = "cannot read PCM wav"; return; }
    if (ch > 1 && (flags & SD_WAV_DOWNMIX)) {
        // the buffer holds all n * ch interleaved samples (the reference keeps the first n of them as "mono", wav.h:95-97)
        for (int64_t i = 0; i < w.n; ++i) {
            float s = 0.0f;
            for (int q = 0; q < ch; ++q) s += w.f32[i * ch + q];
            w.f32[i] = s / (float)ch;
        }
    }
    if (w.sr == 16000 || (flags & SD_WAV_ASSUME_16K)) { w.kind = WavLoad::F32; return; }
    if (!(flags & SD_WAV_RESAMPLE)) {
        w.kind = WavLoad::OFF_RATE;
        w.msg = "sample rate " + std::to_string(w.sr) + " Hz; the pipeline needs 16000 (README.md:37 of the reference, which would process the file as if it "
                "were 16 kHz: SD_WAV_ASSUME_16K / --assume-16k does the same) -- pass SD_WAV_RESAMPLE / --resample";
        return;
    }
    if (w.n <= 0) { w.kind = WavLoad::NO_SAMPLES; w.msg = "holds no samples"; return; }
    w.kind = WavLoad::F32_OFF_RATE;
}

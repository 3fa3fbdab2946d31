// The wav reader and the loading rule of csrc/wav_file.h -- the header walk takes its seeks and sizes from the file -- for AddressSanitizer + UBSan
// on well-formed, streamed, truncated and hostile files.  CPU only; tools/sanitize/build_wav_file.sh builds it.
//   wav_file FILE...   -> per file, one line for each reader and one for the loader under each flag set:
//     <file> pcm16 rc=<code> n=<n> sr=<rate> ch=<channels> <hex of the n * max(ch, 1) int16 samples>
//     <file> f32 rc=<code> n=<n> sr=<rate> ch=<channels> bits=<bits> <hex of the n * max(ch, 1) floats>
//     <file> load flags=<SD_WAV_*> kind=<WavLoad::Kind> n=<n> sr=<rate> <hex of the n samples delivered | the refusal's message>
//   then "wav_file ok" and exit 0
#include <cstdio>
#include "wav_file.h"

static void hex(const void* p, size_t bytes)
{
    for (size_t i = 0; i < bytes; ++i) printf("%02x", ((const unsigned char*)p)[i]);
    if (!bytes) printf("-");
    printf("\n");
}

int main(int argc, char** argv)
{
    for (int k = 1; k < argc; ++k) {
        const char* path = argv[k];
        int16_t* pcm = nullptr; float* wav = nullptr; int64_t n = 0; int32_t sr = 0, ch = 0, bits = 0;
        int rc = wav_read_pcm16(path, &pcm, &n, &sr, &ch);
        printf("%s pcm16 rc=%d n=%lld sr=%d ch=%d ", path, rc, (long long)n, sr, ch);
        hex(pcm, rc == SD_OK ? (size_t)n * (ch > 1 ? ch : 1) * 2 : 0);
        free(pcm);
        n = 0; sr = ch = 0;
        rc = wav_read_f32(path, &wav, &n, &sr, &ch, &bits);
        printf("%s f32 rc=%d n=%lld sr=%d ch=%d bits=%d ", path, rc, (long long)n, sr, ch, bits);
        hex(wav, rc == SD_OK ? (size_t)n * (ch > 1 ? ch : 1) * 4 : 0);
        free(wav);
        for (int flags : {0, SD_WAV_RESAMPLE, SD_WAV_DOWNMIX, SD_WAV_ASSUME_16K, SD_WAV_DOWNMIX | SD_WAV_ASSUME_16K}) {
            WavLoad f;
            wav_load(path, flags, f);
            printf("%s load flags=%d kind=%d n=%lld sr=%d ", path, flags, (int)f.kind, (long long)f.n, f.sr);
            if (f.refused()) printf("%s\n", f.msg.c_str());
            else if (f.kind == WavLoad::PCM16) hex(f.pcm, (size_t)f.n * 2);
            else hex(f.f32, (size_t)f.n * 4);
        }
    }
    printf("wav_file ok\n");
    return 0;
}

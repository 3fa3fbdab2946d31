#!/bin/bash
# CPU-only sanitizer build of the wav reader and the file loading rule (csrc/wav_file.h: the header walk over untrusted files, both readers, the
# --resample / --downmix / --assume-16k rule): AddressSanitizer + UBSan.  Never loaded into python, never run on a GPU.
#   tools/sanitize/build_wav_file.sh <out-binary>;   <out-binary> FILE...   -> what each reader and the loader make of each file, "wav_file ok" and exit 0;
#   sanitizer reports go to stderr
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd)
src=$root/pyannote-audio_speaker-diarization_cpp_amd/csrc
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I$src -I$root/include $here/wav_file_main.cpp -o "$1"

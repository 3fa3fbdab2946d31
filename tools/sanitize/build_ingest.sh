#!/bin/bash
# CPU-only sanitizer build of the planner of sd_diarize_many_audio* (csrc/ingest_plan.h) and of the reader sd_read_wav_audio (csrc/wav_file.h):
# AddressSanitizer + UBSan.  Never loaded into python, never run on a GPU.
#   tools/sanitize/build_ingest.sh <out-binary>;   <out-binary> FILE...   -> what the reader makes of each file, the planner's rounds and limits,
#   "ingest ok" and exit 0; sanitizer reports go to stderr
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd)
src=$root/pyannote-audio_speaker-diarization_cpp_amd/csrc
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I$src -I$root/include $here/ingest_main.cpp -o "$1"

#!/bin/bash
# CPU-only sanitizer build of the planner of sd_stream_push_audio* / sd_stream_push_many_audio* (csrc/stream_ingest_plan.h): AddressSanitizer + UBSan.
# Never loaded into python, never run on a GPU.
#   tools/sanitize/build_stream_ingest.sh <out-binary>;   <out-binary>   -> the named cases, the refusals, 300 random rounds against a naive second
#   implementation, "stream ingest ok" and exit 0; sanitizer reports go to stderr
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd)
src=$root/pyannote-audio_speaker-diarization_cpp_amd/csrc
/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -I$src -I$root/include $here/stream_ingest_main.cpp -o "$1"
